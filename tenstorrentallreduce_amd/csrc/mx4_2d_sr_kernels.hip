// mx4_2d_sr_kernels.hip — the 2D MXFP4 all-gather whose COLUMN-WISE rows are rounded stochastically, with or
// without the random Hadamard rotation in front (allred_plan_all_gather_shards_mxfp4_2d_sr, allred.h): the
// operand of dX = dY W — the one rotation and SR were built for — from the pass that holds every fp32 master
// value in a register anyway, next to the unrotated RNE row-wise rows of the forward GEMM.  No fp32 W^T for the
// 1D SR call, no pass over every rank's copy.
//
//   k_ag_group_mxfp4_2d_sr<P, RCEIL, ROWS, RHT>   k_ag_group_mxfp4_2d's strip walk, images and stores
//                                                 (mx4_2d_kernels.hip); behind a square's barrier the rotation of
//                                                 mx_rht.hpp where RHT and mx_sr.hpp's rounding in place of
//                                                 v_cvt_scalef32_pk_fp4_f32; the square's random words are
//                                                 generated in front of the barrier.
//
// The t rows are bit for bit what k_ag_group_mxfp4_sr writes from a shard that holds W^T; the rows are
// k_ag_group_mxfp4_2d's.  The tests compare whole buffers.  No inline assembly and no hand-written wait here
// beyond lds_barrier() (device.hpp).
#include <type_traits>

#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx2d_image.hpp"
#include "mx4_2d_span.hpp"
#include "mx_quant.hpp"
#include "mx_rht.hpp"
#include "mx_sr.hpp"

namespace tsa {
namespace {

constexpr int kMx4SrGroupMax = ALLRED_MX4_2D_SR_GROUP_MAX;   // buckets of one launch
constexpr int kS = 1 << kMx4LgStrip;                         // row groups of a strip
constexpr int kStripSquares = 1 << kMx4LgSquares;            // 32 x 32 squares of the largest strip

// mx4_2d_kernels.hip's table entry, restated (that file and its ISA stay as they are): entry i for bucket i of
// the launch; GroupSpan carries the row-wise element rows, GroupBucket::ranks the bucket's row 0 of BYTES
// (nullptr: no row-wise outputs) and GroupBucket::stride its row stride in BYTES.  The state's address, the sign
// mask and the launch's first list index travel behind the two tables: 2064 + 20 x 96 + 16 = 4000 bytes.
struct Mx4SrEntry {
    const float* shard;
    uint64_t shard_stride;     // floats
    uint8_t* scales;
    uint64_t scale_stride;     // bytes
    uint8_t* t_rows;
    uint64_t t_row_stride;     // bytes
    uint8_t* t_scales;
    uint64_t t_scale_stride;   // bytes
    Mx4Shape shape;
};
struct Mx4SrTable {
    Mx4SrEntry e[kMx4SrGroupMax];   // entries past the last bucket: zero
};
constexpr size_t kMx4SrTail = sizeof(const allred_mx_sr_state*) + 2 * sizeof(uint32_t);
static_assert(sizeof(Mx4SrEntry) == 96 && sizeof(Mx4SrTable) == 96 * kMx4SrGroupMax, "the kernel-argument layout");
static_assert(sizeof(GroupSpan) + sizeof(Mx4SrTable) + kMx4SrTail < 4096, "kernel arguments stay below 4 KiB");
static_assert(sizeof(GroupSpan) + sizeof(Mx4SrTable) + kMx4SrTail + sizeof(Mx4SrEntry) >= 4096,
              "ALLRED_MX4_2D_SR_GROUP_MAX is the largest count that fits");
static_assert(kMx4SrGroupMax >= 16 && kMx4SrGroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_mx2d_bucket_f32) == 96, "allred.h's layout");

// the launcher's side table: the kernel's table and whether a member of the pending launch has row-wise rows
struct Mx4SrSide {
    Mx4SrTable tab;
    bool rows;
};

// k_ag_group_mxfp4_2d's image, restated: one strip's nibbles as they leave, both element images and both scale
// images, plain linear.  2 x (8 KiB + 8 KiB + 1 KiB) for the two rotating images.
struct alignas(16) Mx4Image {
    uint8_t rows[512 * kStripSquares];    // element (i, j) of the strip is nibble i * 32 sw + j
    uint8_t t[512 * kStripSquares];       // element (i, j) of the strip is nibble j * 32 S + i
    uint8_t rscale[32 * kStripSquares];   // row i's sw scale bytes at i * sw
    uint8_t tscale[32 * kStripSquares];   // column j's S scale bytes at j * S
};
static_assert(2 * sizeof(Mx4Image) + 2 * 32 * kFStride * sizeof(float) <= 48 * 1024, "three workgroups of static LDS per CU");

struct Quant4 {
    uint32_t nibbles;   // four e2m1 nibbles in bits 15:0, element 0 lowest
    uint32_t scale;     // the block's E8M0 byte
};

// what both quantisers share: A over the eight aligned lanes of a block (quant8's three DPP steps), the special
// block, the scale byte and 2^-X — k_ag_group_mxfp4's integer work
struct Scale4 {
    bool special;
    int sb;
    float inv;
};
template <bool RCEIL>
__device__ __forceinline__ Scale4 scale8_fp4(const f32x4& x) {
    uint32_t A = amax4(x);
    A = max_dpp<0xB1>(A);    // quad_perm [1, 0, 3, 2]: lane ^ 1
    A = max_dpp<0x4E>(A);    // quad_perm [2, 3, 0, 1]: lane ^ 2
    A = max_dpp<0x141>(A);   // row_half_mirror: a lane of the other quad of the 8
    int sb = (int)(A >> 23) - 2;
    if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x400000u ? 1 : 0;
    sb = sb > 0 ? sb : 0;
    return Scale4{A >= 0x7f800000u, sb, __uint_as_float((uint32_t)(254 - sb) << 23)};
}

// the ROW-WISE quantiser: k_ag_group_mxfp4_2d's quant8_fp4 — RNE, unrotated
template <bool RCEIL>
__device__ __forceinline__ Quant4 quant8_fp4(const f32x4& x) {
    const Scale4 s = scale8_fp4<RCEIL>(x);
    uint32_t v = cvt2_fp4<0>(x[0] * s.inv, x[1] * s.inv, 0u);
    v = cvt2_fp4<1>(x[2] * s.inv, x[3] * s.inv, v);
    return Quant4{s.special ? 0u : v, s.special ? 0xffu : (uint32_t)s.sb};
}

// the COLUMN-WISE quantiser: 32 consecutive elements of a t row held as four per lane by eight aligned lanes,
// lane c = lane & 7 elements 4 c .. 4 c + 3 — adamw_body.hpp's RHT / SR output stage.
//   RHT   the signs and h = 1, 2 on the lane's four registers (rht_own<4>); h = 4: lane ^ 1, h = 8: lane ^ 2,
//         h = 16: lane ^ 4 — row_half_mirror composed with quad_perm [3, 2, 1, 0], i ^ 7 ^ 3 —, one v_add_f32
//         with a DPP operand per register and stage; then ONE multiply by 2^-2.5.  The rule's order: the bits are
//         k_ag_group_mxfp4_sr's.
//   SR    A, the special block, the scale byte and 2^-X on the (rotated) values as above, then sr4_fp4 with the
//         lane's ONE Philox result: no clamp, the rule saturates.
template <bool RCEIL, bool RHT>
__device__ __forceinline__ Quant4 quant8_fp4_sr(f32x4 y, const RhtLane<4>& rl, const SrWords& rnd) {
    if constexpr (RHT) {
        float x[4] = {y[0], y[1], y[2], y[3]};
        rht_own(x, rl);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x[e] = rht_pair(dpp_f<0xB1>(x[e]), x[e], rl.upper[0]);                  // h = 4: lane ^ 1
            x[e] = rht_pair(dpp_f<0x4E>(x[e]), x[e], rl.upper[1]);                  // h = 8: lane ^ 2
            x[e] = rht_pair(dpp_f<0x1B>(dpp_f<0x141>(x[e])), x[e], rl.upper[2]);    // h = 16: lane ^ 4
            y[e] = rht_norm(x[e]);
        }
    }
    const Scale4 s = scale8_fp4<RCEIL>(y);
    const uint32_t v = sr4_fp4(y, s.inv, rnd);
    return Quant4{s.special ? 0u : v, s.special ? 0xffu : (uint32_t)s.sb};
}

// ---------------------------------------------------------------------------
// k_ag_group_mxfp4_2d_sr<P, RCEIL, ROWS, RHT>: k_ag_group_mxfp4_2d line for line — the persistent grid, the
// forward-only wave-uniform cursor, strips of S x sw squares of the MATRIX taken square by square, thread tid
// holding floats 4 c .. 4 c + 3 (c = tid & 7) of row r = tid >> 3 of the square, the next square's load in front
// of this one's arithmetic, the row-wise phase (RNE), F[n & 1], the two rotating images and both store stages —
// with a column phase of its own.
//   THE WORDS.  Behind the barrier thread tid holds rows 4 c .. 4 c + 3 of column r of the square: with J the
//   matrix column j0 + 32 qj + r and G the row group g0 + qi, elements e = J nrows + 32 G + 4 c .. + 3 of the t
//   row — four consecutive positions, e % 4 == 0 (nrows % 256 == 0): ONE Philox call, counter g = e / 4 =
//   J (nrows / 4) + 8 G + c, the words in element order.  g depends on indices alone, so the call stands IN
//   FRONT of the square's barrier, behind the F store: its ~85 integer operations run while the wave's LDS
//   writes land and the slower waves arrive, not behind the barrier in front of the quantiser, where every wave
//   would run them with the transposed floats already waiting.  Two sched_barriers hold it there.  The unit's
//   part of g — (j0 + 32 qj) (nrows / 4) + 8 G — is scalar 64-bit arithmetic; r (nrows / 4) is per thread and
//   computed once, in front of the unit loop's squares.  The key, the step and the bucket's list index
//   (first_bucket + its slot) are wave-uniform; the state is read ONCE per wave, through the scalar cache.
//   Four words are live across the barrier.
//   THE ROUNDING.  quant8_fp4_sr above.  Each element of W is rounded once here — by the one thread that holds
//   it behind the transpose — not once per storing wave as in k_ag_group_mxfp4_sr.
// LDS hazards: k_ag_group_mxfp4_2d's argument unchanged — the column phase reads F and writes the image's t and
// tscale bytes at the same places, behind the same barrier; the words live in registers.
// ---------------------------------------------------------------------------
template <int P, bool RCEIL, bool ROWS, bool RHT>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp4_2d_sr(GroupSpan span, Mx4SrTable tab,
                                                                 const allred_mx_sr_state* __restrict__ sr, uint32_t sign_mask,
                                                                 uint32_t first_bucket) {
    constexpr int RPW = P / 4;
    constexpr uint32_t LGT = 4 + kMx4LgStrip;   // bytes of a column of the t image, as a shift: 16 S
    static_assert(P == 8 || P == 16 || P == 32 || P == 64, "P = 8, 16, 32 or 64");
    __shared__ Mx4Image image[2];
    __shared__ __attribute__((aligned(16))) float F[2][32 * kFStride];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = tid >> 3, c = tid & 7;
    const SrCall call = sr_call(sr);
    RhtLane<4> rl{};
    if constexpr (RHT) rl = rht_lane<4>(sign_mask, c);
    struct Unit {          // copies, not pointers into the by-value tables: those stay in the kernel-argument segment
        uint8_t* rows;     // the bucket's row-wise element row 0, or nullptr
        uint64_t row_stride;
        Mx4SrEntry e;
        Mx4Unit at;
        uint32_t bucket;   // index in the CALLER's list
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& b = span.b[gt.bucket];
        const Mx4SrEntry& e = tab.e[gt.bucket];
        return Unit{reinterpret_cast<uint8_t*>(b.ranks), b.stride, e, mx4_2d_unit_at(e.shape, gt.block, gt.rem),
                    first_bucket + gt.bucket};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;
    const int last = mine - 1;
    auto load = [&](const Unit& u, uint32_t q) {
        const Mx4Shape& s = u.e.shape;
        const Mx4Group g = mx4_2d_group_at(s, u.at.g0 + (q >> s.lgw), u.e.shard_stride);
        const uint64_t j = u.at.j0 + ((uint64_t)(q & ((1u << s.lgw) - 1)) << 5) + 4u * (uint32_t)c;
        return *reinterpret_cast<const f32x4*>(u.e.shard + g.src + (uint64_t)r * s.cols + j);
    };
    uint32_t staged = 0;
    f32x4 x = load(locate(0), 0);
    for (int j = 0; j < mine; ++j) {
        // located again, not carried over from the prefetch below (k_ag_group_mxfp8_2d: a Unit that lives across
        // iterations ends up in scratch, and the second walk of the same unit is scalar work)
        const Unit cu = locate(j);
        const uint32_t lgw = cu.e.shape.lgw, squares = (uint32_t)kS << lgw;
        Mx4Image& img = image[j & 1];
        const bool rows = ROWS && cu.rows != nullptr;   // uniform over the workgroup
        // g of the thread's first element of square (qi, qj): unit_g + (32 qj) quarter + 8 qi + mine_g
        const uint64_t quarter = cu.e.shape.nrows >> 2;
        const uint64_t unit_g = cu.at.j0 * quarter + 8u * (uint64_t)cu.at.g0;   // scalar
        const uint64_t mine_g = (uint64_t)(uint32_t)r * quarter + (uint32_t)c;
        for (uint32_t q = 0; q < squares; ++q) {
            f32x4 nx;
            if (q + 1 < squares) {
                nx = load(cu, q + 1);
            } else {
                nx = load(locate(j < last ? j + 1 : last), 0);
            }
            const uint32_t qi = q >> lgw, qj = q & ((1u << lgw) - 1);
            float* f = F[staged & 1];
            ++staged;
            *reinterpret_cast<f32x4*>(f + r * kFStride + 4 * c) = x;
            __builtin_amdgcn_sched_barrier(0);   // the next square's load and the F store are out
            const uint64_t g = unit_g + ((uint64_t)(32u * qj) * quarter + 8u * qi) + mine_g;
            // the key is made opaque per square: the nine bumped key pairs are then 18 s_add_u32 here, not 18 scalar
            // registers kept across the whole walk — with those 17 of the 32 instances spilt 8 to 16 SGPRs
            SrCall sq = call;
            asm volatile("" : "+s"(sq.k0), "+s"(sq.k1));
            const SrWords rnd = sr_words(sq, (uint32_t)g, (uint32_t)(g >> 32), cu.bucket);
            __builtin_amdgcn_sched_barrier(0);   // the words stand in front of the barrier
            if (rows) {
                const Quant4 a = quant8_fp4<RCEIL>(x);
                const uint32_t i = 32 * qi + (uint32_t)r;
                *reinterpret_cast<uint16_t*>(img.rows + ((i << (4 + lgw)) + 16 * qj + 2 * (uint32_t)c)) = (uint16_t)a.nibbles;
                if (c == 0) img.rscale[(i << lgw) + qj] = (uint8_t)a.scale;
            }
            lds_barrier();
            const f32x4 y = {f[(4 * c + 0) * kFStride + r], f[(4 * c + 1) * kFStride + r], f[(4 * c + 2) * kFStride + r],
                             f[(4 * c + 3) * kFStride + r]};
            const Quant4 a = quant8_fp4_sr<RCEIL, RHT>(y, rl, rnd);
            const uint32_t jj = 32 * qj + (uint32_t)r;
            *reinterpret_cast<uint16_t*>(img.t + ((jj << LGT) + 16 * qi + 2 * (uint32_t)c)) = (uint16_t)a.nibbles;
            if (c == 0) img.tscale[(jj << kMx4LgStrip) + qi] = (uint8_t)a.scale;
            x = nx;
        }
        lds_barrier();
        const uint64_t cols = cu.e.shape.cols, nrows = cu.e.shape.nrows;
        // 512 bytes of each image per square, 1 KiB per instruction: squares / 2 trips (squares >= S is even)
        for (uint32_t i = 0; i < squares / 2; ++i) {
            const uint32_t o = i * 1024 + 16 * (uint32_t)lane;
            if (rows) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(img.rows + o);
                uint8_t* p = cu.rows + cu.at.row + (uint64_t)(o >> (4 + lgw)) * (cols >> 1) + (o & ((16u << lgw) - 1));
#pragma unroll
                for (int k = 0; k < RPW; ++k)
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p + (uint64_t)(RPW * w + k) * cu.row_stride));
            }
            const u32x4 v = *reinterpret_cast<const u32x4*>(img.t + o);
            uint8_t* p = cu.e.t_rows + cu.at.t + (uint64_t)(o >> LGT) * (nrows >> 1) + (o & ((1u << LGT) - 1));
#pragma unroll
            for (int k = 0; k < RPW; ++k)
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p + (uint64_t)(RPW * w + k) * cu.e.t_row_stride));
        }
        // the scale bytes: row i's sw bytes, column j's S bytes; NOT nontemporal (k_ag_group_mxfp8's finding)
        if (rows) {
            for (uint32_t i = (uint32_t)lane; i < 32u * kS; i += 64) {
                uint8_t* p = cu.e.scales + cu.at.rscale + (uint64_t)i * (cols >> 5);
                for (int k = 0; k < RPW; ++k) put_scales(p + (uint64_t)(RPW * w + k) * cu.e.scale_stride, img.rscale + (i << lgw), lgw);
            }
        }
        using StripScales = std::conditional_t<kS == 4, uint32_t, uint64_t>;   // a column's S scale bytes, ONE store
        for (uint32_t i = (uint32_t)lane; i < (32u << lgw); i += 64) {
            uint8_t* p = cu.e.t_scales + cu.at.tscale + (uint64_t)i * (nrows >> 5);
            const StripScales v = *reinterpret_cast<const StripScales*>(img.tscale + (i << kMx4LgStrip));
            for (int k = 0; k < RPW; ++k) *reinterpret_cast<StripScales*>(p + (uint64_t)(RPW * w + k) * cu.e.t_scale_stride) = v;
        }
    }
}
// k_ag_group_mxfp4_2d's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAgGroupMx4_2dSrGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx2d_check with the MXFP4 payload, then sr's own rules) list of buckets — one fp32 matrix
// each, in shard blocks — through k_ag_group_mxfp4_2d_sr, ALLRED_MX4_2D_SR_GROUP_MAX buckets per launch in list
// order.  Every bucket is a member, so launch `index` begins at bucket index * ALLRED_MX4_2D_SR_GROUP_MAX of the
// caller's list: the counter's third word does not depend on the batching.  dry: nothing is launched and the
// number of launches is returned.
int launch_ag_group_mxfp4_2d_sr(const allred_mx2d_bucket_f32* buckets, int count, int total, bool rceil, bool rotate,
                                uint32_t sign_mask, const allred_mx_sr_state* sr, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Mx4SrSide side{};
    auto add = [&](int i, int slot) {
        const allred_mx2d_bucket_f32& b = buckets[i];
        Mx4Shape shape;
        uint64_t cgs, all;
        // the caller's checks, kept next to their use
        if (total < 8 || b.cols == 0 || b.elems_per_rank % b.cols ||
            !mx4_2d_shape_make(&shape, b.cols, b.elems_per_rank / b.cols, (uint64_t)total, &cgs, &all))
            return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);
        side.tab.e[slot] = Mx4SrEntry{b.shard, b.shard_stride, b.scales, b.scale_stride, b.t_rows, b.t_row_stride,
                                      b.t_scales, b.t_scale_stride, shape};
        side.rows = side.rows || b.rows != nullptr;
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, all, cgs});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t) {
        const bool rows = side.rows;
        const uint32_t first = (uint32_t)index * kMx4SrGroupMax;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto rc, auto rw, auto rot) {
                hipLaunchKernelGGL((k_ag_group_mxfp4_2d_sr<p(), decltype(rc)::value, decltype(rw)::value, decltype(rot)::value>),
                                   dim3(grid), dim3(kBlock), 0, st, span, side.tab, sr, sign_mask, first);
                trace_launch(grid, kBlock, "k_ag_group_mxfp4_2d_sr<%d, %s, %s, %s>", total, tf(rceil), tf(rows), tf(rotate));
            };
            auto with_rows = [&](auto rc, auto rot) {
                if (rows) go(rc, std::true_type{}, rot);
                else go(rc, std::false_type{}, rot);
            };
            if (rceil) {
                if (rotate) with_rows(std::true_type{}, std::true_type{});
                else with_rows(std::true_type{}, std::false_type{});
            } else {
                if (rotate) with_rows(std::false_type{}, std::true_type{});
                else with_rows(std::false_type{}, std::false_type{});
            }
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMx4SrGroupMax>(count, dry, side, add,
                                       [](uint64_t units) { return persistent_grid(units, kAgGroupMx4_2dSrGrid); }, launch);
}

}  // namespace tsa
