// mx4_2d_kernels.hip — the grouped all-gather from fp32 shards into BOTH MXFP4 orientations of a weight
// (allred_plan_all_gather_shards_mxfp4_2d, allred.h): the row-wise nibble rows allred_plan_all_gather_shards_mxfp4
// writes (MX blocks along `cols`, the operand of Y = X W^T) and the column-wise rows — W^T in the same
// plain-linear MXFP4 row format, MX blocks along the rows of W, the operand of dX = dY W — from ONE read of
// the fp32 masters.  Both are rounded once, from the fp32 value.
//
//   k_ag_group_mxfp4_2d<P, RCEIL, ROWS>   the persistent grouped walk (group_span.hpp) over STRIPS of the
//                                         matrix (mx4_2d_span.hpp): S consecutive 32-row groups, taken from
//                                         as many neighbouring shard blocks as they lie in, by up to 128
//                                         columns; ROWS = false: no bucket of the launch has row-wise rows.
//
// Why strips.  At four bits per element a patch of ONE shard block of R rows leaves in t runs of R / 2 bytes:
// 16 bytes at R = 32.  The rows of neighbouring shard blocks are neighbours in every t row, so a unit that
// takes its row groups across block ends writes runs of 16 S bytes whatever R is.
// The quantisation is k_ag_group_mxfp4's, bit for bit: mx_quant.hpp's helpers, ONE fp32 multiply by a power
// of two with denormals kept, v_med3_f32 and v_cvt_scalef32_pk_fp4_f32 at scale 1.0, everything around them
// integer work.  No inline assembly and no hand-written wait here beyond lds_barrier() (device.hpp).
#include <type_traits>

#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx2d_image.hpp"
#include "mx4_2d_span.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

constexpr int kMx4GroupMax = ALLRED_MX4_2D_GROUP_MAX;   // buckets of one launch
constexpr int kS = 1 << kMx4LgStrip;                    // row groups of a strip
constexpr int kStripSquares = 1 << kMx4LgSquares;       // 32 x 32 squares of the largest strip

// Entry i for bucket i of the launch.  GroupSpan carries the row-wise element rows: GroupBucket::ranks is the
// bucket's row 0 of BYTES (nullptr: the bucket has no row-wise outputs) and GroupBucket::stride its row
// stride in BYTES.  96 bytes per entry: 2064 + 21 x 96 = 4080 bytes of kernel arguments.
struct Mx4Entry {
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
struct Mx4Table {
    Mx4Entry e[kMx4GroupMax];   // entries past the last bucket: zero
};
static_assert(sizeof(Mx4Entry) == 96 && sizeof(Mx4Table) == 96 * kMx4GroupMax, "the kernel-argument layout");
static_assert(sizeof(GroupSpan) + sizeof(Mx4Table) < 4096, "kernel arguments stay below 4 KiB");
static_assert(sizeof(GroupSpan) + sizeof(Mx4Table) + sizeof(Mx4Entry) >= 4096, "ALLRED_MX4_2D_GROUP_MAX is the largest count that fits");
static_assert(kMx4GroupMax >= 16 && kMx4GroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_mx2d_bucket_f32) == 96, "allred.h's layout");

// the launcher's side table: the kernel's table and whether a member of the pending launch has row-wise rows
struct Mx4Side {
    Mx4Table tab;
    bool rows;
};

// one strip's quantised nibbles as they leave: both element images and both scale images, plain linear.
// 512 bytes of each element image per square: 2 x (8 KiB + 8 KiB + 1 KiB) for the two rotating images.
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

// allred.h's MXFP4 rule for 32 consecutive floats held as four per lane by EIGHT aligned lanes — the
// reduction of quant8 (mx2d_image.hpp), three DPP steps, then k_ag_group_mxfp4's arithmetic unchanged.
// BOTH directions of a square go through it: a row block before the transpose, a column block behind it.
template <bool RCEIL>
__device__ __forceinline__ Quant4 quant8_fp4(const f32x4& x) {
    uint32_t A = amax4(x);
    A = max_dpp<0xB1>(A);    // quad_perm [1, 0, 3, 2]: lane ^ 1
    A = max_dpp<0x4E>(A);    // quad_perm [2, 3, 0, 1]: lane ^ 2
    A = max_dpp<0x141>(A);   // row_half_mirror: a lane of the other quad of the 8
    const bool special = A >= 0x7f800000u;
    int sb = (int)(A >> 23) - 2;
    if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x400000u ? 1 : 0;
    sb = sb > 0 ? sb : 0;
    const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
    uint32_t v = cvt2_fp4<0>(x[0] * inv, x[1] * inv, 0u);
    v = cvt2_fp4<1>(x[2] * inv, x[3] * inv, v);
    return Quant4{special ? 0u : v, special ? 0xffu : (uint32_t)sb};
}

// ---------------------------------------------------------------------------
// k_ag_group_mxfp4_2d<P, RCEIL, ROWS>: a persistent grid, workgroup g takes units g + j * G through a
// forward-only wave-uniform cursor over GroupSpan, as k_ag_group_mxfp8_2d does.  A unit is a strip of
// S x sw squares of the MATRIX (mx4_2d_span.hpp), taken square by square, square q at row group q >> lgw of
// the strip and column square q & (sw - 1); the row group's shard block comes from mx4_2d_group_at per square
// (wave-uniform: one multiply by the host's reciprocal and one correction).  Thread tid holds floats
// 4 c .. 4 c + 3 (c = tid & 7) of row r = tid >> 3 of the square, loaded with one 16-byte load, the next
// square's (the next unit's first, at a strip's end; a workgroup's last unit once more) before this one's
// arithmetic.  Per square:
//   row-wise     the thread's four floats are a quarter of a row block of eight aligned lanes: quant8_fp4;
//                its four nibbles are TWO WHOLE BYTES of the image's `rows` — one 2-byte LDS store, no byte
//                shared between threads —, lane c = 0's scale byte goes to `rscale`;
//   the floats   go to F[n & 1], 32 rows of kFStride floats, n the squares this workgroup has staged;
//   barrier;
//   column-wise  thread tid reads rows 4 c .. 4 c + 3 of column r of F[n & 1]: a quarter of a column block
//                of eight aligned lanes, four CONSECUTIVE elements of the t row: quant8_fp4 again, two whole
//                bytes to `t`, lane c = 0's scale byte to `tscale`.
// Behind the strip's last square: barrier; every wave streams BOTH nibble images, 16 bytes per lane and
// 1 KiB per instruction, with nontemporal stores to its P / 4 rank rows and t rows — runs of 16 sw bytes
// in a row, of 16 S bytes in a t row —, and the scale images with plain stores (mx_kernels.hip says why)
// of sw or S bytes.
// LDS hazards.  F is written in front of a square's barrier and read behind it; F[n & 1] is written
// again at square n + 2, and between a wave's read at square n and any wave's write at square n + 2
// lies the barrier of square n + 1, which no wave passes before every wave has arrived, i.e. has done
// its reads of square n.  The image rotates the same way with the unit's index j: image[j & 1] is
// written during unit j (the row-wise bytes in front of a square's barrier, the t bytes behind it), read
// behind unit j's last barrier, and written again during unit j + 2, after the S sw >= 4 barriers of unit
// j + 1, which every wave reaches only behind its reads of unit j.  Between the writes and the reads of
// one image lies the unit's last barrier.  Inside an image no byte has two writers: a thread's four
// nibbles are bytes 2 c and 2 c + 1 of its row's (column's) 16 bytes of the square.
// ---------------------------------------------------------------------------
template <int P, bool RCEIL, bool ROWS>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp4_2d(GroupSpan span, Mx4Table tab) {
    constexpr int RPW = P / 4;
    constexpr uint32_t LGT = 4 + kMx4LgStrip;   // bytes of a column of the t image, as a shift: 16 S
    static_assert(P == 8 || P == 16 || P == 32 || P == 64, "P = 8, 16, 32 or 64");
    __shared__ Mx4Image image[2];
    __shared__ __attribute__((aligned(16))) float F[2][32 * kFStride];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = tid >> 3, c = tid & 7;
    struct Unit {          // copies, not pointers into the by-value tables: those stay in the kernel-argument segment
        uint8_t* rows;     // the bucket's row-wise element row 0, or nullptr
        uint64_t row_stride;
        Mx4Entry e;
        Mx4Unit at;
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& b = span.b[gt.bucket];
        const Mx4Entry& e = tab.e[gt.bucket];
        return Unit{reinterpret_cast<uint8_t*>(b.ranks), b.stride, e, mx4_2d_unit_at(e.shape, gt.block, gt.rem)};
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
            if (rows) {
                const Quant4 a = quant8_fp4<RCEIL>(x);
                const uint32_t i = 32 * qi + (uint32_t)r;
                *reinterpret_cast<uint16_t*>(img.rows + ((i << (4 + lgw)) + 16 * qj + 2 * (uint32_t)c)) = (uint16_t)a.nibbles;
                if (c == 0) img.rscale[(i << lgw) + qj] = (uint8_t)a.scale;
            }
            lds_barrier();
            const f32x4 y = {f[(4 * c + 0) * kFStride + r], f[(4 * c + 1) * kFStride + r], f[(4 * c + 2) * kFStride + r],
                             f[(4 * c + 3) * kFStride + r]};
            const Quant4 a = quant8_fp4<RCEIL>(y);
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
// k_ag_group_f32's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAgGroupMx4_2dGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx2d_check with the MXFP4 payload) list of buckets — one fp32 matrix each, in
// shard blocks — through k_ag_group_mxfp4_2d, ALLRED_MX4_2D_GROUP_MAX buckets per launch in list order.
// dry: nothing is launched and the number of launches is returned.
int launch_ag_group_mxfp4_2d(const allred_mx2d_bucket_f32* buckets, int count, int total, bool rceil, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Mx4Side side{};
    auto add = [&](int i, int slot) {
        const allred_mx2d_bucket_f32& b = buckets[i];
        Mx4Shape shape;
        uint64_t cgs, all;
        // the caller's checks, kept next to their use
        if (total < 8 || b.cols == 0 || b.elems_per_rank % b.cols ||
            !mx4_2d_shape_make(&shape, b.cols, b.elems_per_rank / b.cols, (uint64_t)total, &cgs, &all))
            return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);
        side.tab.e[slot] = Mx4Entry{b.shard, b.shard_stride, b.scales, b.scale_stride, b.t_rows, b.t_row_stride,
                                    b.t_scales, b.t_scale_stride, shape};
        side.rows = side.rows || b.rows != nullptr;
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, all, cgs});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int, uint64_t) {
        const bool rows = side.rows;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, span, side.tab);
                trace_launch(grid, kBlock, "k_ag_group_mxfp4_2d<%d, %s, %s>", total, tf(rceil), tf(rows));
            };
            if (rceil) rows ? go(k_ag_group_mxfp4_2d<p(), true, true>) : go(k_ag_group_mxfp4_2d<p(), true, false>);
            else rows ? go(k_ag_group_mxfp4_2d<p(), false, true>) : go(k_ag_group_mxfp4_2d<p(), false, false>);
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMx4GroupMax>(count, dry, side, add, [](uint64_t units) { return persistent_grid(units, kAgGroupMx4_2dGrid); },
                                     launch);
}

}  // namespace tsa
