// mx2d_kernels.hip — the grouped all-gather from fp32 shards into BOTH MXFP8 orientations of a weight
// (allred_plan_all_gather_shards_mxfp8_2d, allred.h): the row-wise rows allred_plan_all_gather_shards_mxfp8
// writes (MX blocks along `cols`, the operand of Y = X W^T) and the column-wise rows — W^T in the same
// plain-linear MX row format, MX blocks along the rows of W, the operand of dX = dY W — from ONE read of
// the fp32 masters.  Both are rounded once, from the fp32 value.
//
//   k_ag_group_mxfp8_2d<P, RCEIL, ROWS>   the persistent grouped walk (group_span.hpp) over PATCHES of
//                                         whole 32 x 32 squares (mx2d_span.hpp); ROWS = false: no bucket
//                                         of the launch has row-wise rows.
//
// The quantisation is k_ag_group_mxfp8's, bit for bit: mx_quant.hpp's helpers, ONE fp32 multiply by a
// power of two, everything around it integer work.  No inline assembly and no hand-written wait here
// beyond lds_barrier() (device.hpp).
#include <type_traits>

#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx2d_span.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

constexpr int kMx2dGroupMax = ALLRED_MX2D_GROUP_MAX;   // buckets of one launch

// Entry i for bucket i of the launch.  GroupSpan carries the row-wise element rows: GroupBucket::ranks
// is the bucket's row 0 of BYTES (nullptr: the bucket has no row-wise outputs) and GroupBucket::stride
// its row stride in BYTES.  96 bytes per entry: 2064 + 21 x 96 = 4080 bytes of kernel arguments.
struct Mx2dEntry {
    const float* shard;
    uint64_t shard_stride;     // floats
    uint8_t* scales;
    uint64_t scale_stride;     // bytes
    uint8_t* t_rows;
    uint64_t t_row_stride;     // bytes
    uint8_t* t_scales;
    uint64_t t_scale_stride;   // bytes
    Mx2dShape shape;
};
struct Mx2dTable {
    Mx2dEntry e[kMx2dGroupMax];   // entries past the last bucket: zero
};
static_assert(sizeof(Mx2dEntry) == 96 && sizeof(Mx2dTable) == 96 * kMx2dGroupMax, "the kernel-argument layout");
static_assert(sizeof(GroupSpan) + sizeof(Mx2dTable) < 4096, "kernel arguments stay below 4 KiB");
static_assert(sizeof(GroupSpan) + sizeof(Mx2dTable) + sizeof(Mx2dEntry) >= 4096, "ALLRED_MX2D_GROUP_MAX is the largest count that fits");
static_assert(kMx2dGroupMax >= 16 && kMx2dGroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_mx2d_bucket_f32) == 96, "allred.h's layout");

// the launcher's side table: the kernel's table and whether a member of the pending launch has row-wise rows
struct Mx2dSide {
    Mx2dTable tab;
    bool rows;
};

constexpr int kSquares = 1 << (2 * kMx2dLgSide);   // 32 x 32 squares of the largest patch
constexpr int kFStride = 36;                       // floats between the rows of the staged square: 16-byte aligned rows

// one patch's quantised bytes as they leave: both element images and both scale images, plain linear
struct alignas(16) Mx2dImage {
    uint8_t rows[1024 * kSquares];   // byte (i, j) of the patch at i * 32 sw + j
    uint8_t t[1024 * kSquares];      // byte (i, j) of the patch at j * 32 sh + i
    uint8_t rscale[32 * kSquares];   // row i's sw scale bytes at i * sw
    uint8_t tscale[32 * kSquares];   // column j's sh scale bytes at j * sh
};

struct Quant {
    uint32_t bytes;   // four e4m3fn bytes, element 0 lowest
    uint32_t scale;   // the block's E8M0 byte
};

// allred.h's rule for 32 consecutive floats held as four per lane by EIGHT aligned lanes: the integer
// amax through adamw_body.hpp's three DPP steps, then k_ag_group_mxfp8's arithmetic unchanged
template <bool RCEIL>
__device__ __forceinline__ Quant quant8(const f32x4& x) {
    uint32_t A = umax(umax(abs_bits(x[0]), abs_bits(x[1])), umax(abs_bits(x[2]), abs_bits(x[3])));
    A = max_dpp<0xB1>(A);    // quad_perm [1, 0, 3, 2]: lane ^ 1
    A = max_dpp<0x4E>(A);    // quad_perm [2, 3, 0, 1]: lane ^ 2
    A = max_dpp<0x141>(A);   // row_half_mirror: a lane of the other quad of the 8
    const bool special = A >= 0x7f800000u;
    int sb = (int)(A >> 23) - 8;
    if constexpr (RCEIL) sb += (A & 0x7fffffu) > 0x600000u ? 1 : 0;
    sb = sb > 0 ? sb : 0;
    const float inv = __uint_as_float((uint32_t)(254 - sb) << 23);
    uint32_t v = cvt2<false>(x[0] * inv, x[1] * inv, 0u);
    v = cvt2<true>(x[2] * inv, x[3] * inv, v);
    return Quant{special ? 0x7f7f7f7fu : v, special ? 0xffu : (uint32_t)sb};
}

// `bytes` (1, 2 or 4, wave-uniform) scale bytes from LDS to global memory with ONE plain store
__device__ __forceinline__ void put_scales(uint8_t* dst, const uint8_t* src, uint32_t lg) {
    if (lg == 0) *dst = *src;
    else if (lg == 1) *reinterpret_cast<uint16_t*>(dst) = *reinterpret_cast<const uint16_t*>(src);
    else *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
}

// ---------------------------------------------------------------------------
// k_ag_group_mxfp8_2d<P, RCEIL, ROWS>: a persistent grid, workgroup g takes units g + j * G through a
// forward-only wave-uniform cursor over GroupSpan, as k_ag_group_mxfp8 does.  A unit is a patch of
// sh x sw squares of one shard block (mx2d_span.hpp), taken square by square; thread tid holds floats
// 4 c .. 4 c + 3 (c = tid & 7) of row r = tid >> 3 of the square, loaded with one 16-byte load, the next
// square's (the next unit's first, at a patch's end; a workgroup's last unit once more) before this one's
// arithmetic.  Per square:
//   row-wise     the thread's four floats are a quarter of a row block of eight aligned lanes: quant8; the
//                dword of bytes goes to the image's `rows`, lane c = 0's scale byte to `rscale`.
//   the floats   go to F[n & 1], 32 rows of kFStride floats, n the squares this workgroup has staged;
//   barrier;
//   column-wise  thread tid reads rows 4 c .. 4 c + 3 of column r of F[n & 1]: a quarter of a column block
//                of eight aligned lanes: quant8 again; the dword goes to `t`, lane c = 0's byte to `tscale`.
// Behind the patch's last square: barrier; every wave streams BOTH element images, 16 bytes per lane
// and 1 KiB per instruction, with nontemporal stores to its P / 4 rank rows and t rows, and the scale
// images with plain stores (mx_kernels.hip says why) of sw or sh bytes.
// LDS hazards.  F is written in front of a square's barrier and read behind it; F[n & 1] is written
// again at square n + 2, and between a wave's read at square n and any wave's write at square n + 2
// lies the barrier of square n + 1, which no wave passes before every wave has arrived, i.e. has done
// its reads of square n.  The image rotates the same way with the unit's index j: image[j & 1] is
// written during unit j, read behind unit j's last barrier, and written again during unit j + 2, after
// at least the barriers of unit j + 1, which every wave reaches only behind its reads of unit j.
// Between the writes and the reads of one image lies the unit's last barrier.
// ---------------------------------------------------------------------------
template <int P, bool RCEIL, bool ROWS>
__global__ __launch_bounds__(kBlock) void k_ag_group_mxfp8_2d(GroupSpan span, Mx2dTable tab) {
    constexpr int RPW = P / 4;
    constexpr uint32_t LGP = P == 8 ? 3 : P == 16 ? 4 : P == 32 ? 5 : 6;
    static_assert((1 << LGP) == P, "P = 8, 16, 32 or 64");
    __shared__ Mx2dImage image[2];
    __shared__ __attribute__((aligned(16))) float F[2][32 * kFStride];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = tid >> 3, c = tid & 7;
    struct Unit {          // copies, not pointers into the by-value tables: those stay in the kernel-argument segment
        uint8_t* rows;     // the bucket's row-wise element row 0, or nullptr
        uint64_t row_stride;
        Mx2dEntry e;
        Mx2dUnit at;
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& b = span.b[gt.bucket];
        const Mx2dEntry& e = tab.e[gt.bucket];
        return Unit{reinterpret_cast<uint8_t*>(b.ranks), b.stride, e, mx2d_unit_at(e.shape, gt.block, gt.rem, e.shard_stride, LGP)};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;
    const int last = mine - 1;
    // square q of the unit is (q >> lgw, q & (sw - 1)) in (row, column) squares
    auto load = [&](const Unit& u, uint32_t q) {
        const Mx2dShape& s = u.e.shape;
        const uint64_t i = ((uint64_t)(q >> s.lgw) << 5) + (uint32_t)r, j = ((uint64_t)(q & ((1u << s.lgw) - 1)) << 5) + 4u * (uint32_t)c;
        return *reinterpret_cast<const f32x4*>(u.e.shard + u.at.src + i * s.cols + j);
    };
    uint32_t staged = 0;
    f32x4 x = load(locate(0), 0);
    for (int j = 0; j < mine; ++j) {
        // located again, not carried over from the prefetch below: a Unit that lives across iterations ends up in
        // scratch, and the second walk of the same unit is scalar work (the cursor stands still for it)
        const Unit cu = locate(j);
        const uint32_t lgh = cu.e.shape.lgh, lgw = cu.e.shape.lgw, squares = 1u << (lgh + lgw);
        Mx2dImage& img = image[j & 1];
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
                const Quant a = quant8<RCEIL>(x);
                const uint32_t i = 32 * qi + (uint32_t)r;
                *reinterpret_cast<uint32_t*>(img.rows + ((i << (5 + lgw)) + 32 * qj + 4 * (uint32_t)c)) = a.bytes;
                if (c == 0) img.rscale[(i << lgw) + qj] = (uint8_t)a.scale;
            }
            lds_barrier();
            const f32x4 y = {f[(4 * c + 0) * kFStride + r], f[(4 * c + 1) * kFStride + r], f[(4 * c + 2) * kFStride + r],
                             f[(4 * c + 3) * kFStride + r]};
            const Quant a = quant8<RCEIL>(y);
            const uint32_t jj = 32 * qj + (uint32_t)r;
            *reinterpret_cast<uint32_t*>(img.t + ((jj << (5 + lgh)) + 32 * qi + 4 * (uint32_t)c)) = a.bytes;
            if (c == 0) img.tscale[(jj << lgh) + qi] = (uint8_t)a.scale;
            x = nx;
        }
        lds_barrier();
        const uint64_t cols = cu.e.shape.cols, nrows = cu.e.shape.nrows;
        for (uint32_t i = 0; i < squares; ++i) {
            const uint32_t o = i * 1024 + 16 * (uint32_t)lane;
            if (rows) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(img.rows + o);
                uint8_t* p = cu.rows + cu.at.row + (uint64_t)(o >> (5 + lgw)) * cols +
                             (o & ((32u << lgw) - 1));
#pragma unroll
                for (int k = 0; k < RPW; ++k)
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p + (uint64_t)(RPW * w + k) * cu.row_stride));
            }
            const u32x4 v = *reinterpret_cast<const u32x4*>(img.t + o);
            uint8_t* p = cu.e.t_rows + cu.at.t + (uint64_t)(o >> (5 + lgh)) * nrows + (o & ((32u << lgh) - 1));
#pragma unroll
            for (int k = 0; k < RPW; ++k)
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p + (uint64_t)(RPW * w + k) * cu.e.t_row_stride));
        }
        // the scale bytes: row i's sw bytes, column j's sh bytes; NOT nontemporal (k_ag_group_mxfp8's finding)
        if (rows) {
            for (uint32_t i = (uint32_t)lane; i < (32u << lgh); i += 64) {
                uint8_t* p = cu.e.scales + cu.at.rscale + (uint64_t)i * (cols >> 5);
                for (int k = 0; k < RPW; ++k) put_scales(p + (uint64_t)(RPW * w + k) * cu.e.scale_stride, img.rscale + (i << lgw), lgw);
            }
        }
        for (uint32_t i = (uint32_t)lane; i < (32u << lgw); i += 64) {
            uint8_t* p = cu.e.t_scales + cu.at.tscale + (uint64_t)i * (nrows >> 5);
            for (int k = 0; k < RPW; ++k) put_scales(p + (uint64_t)(RPW * w + k) * cu.e.t_scale_stride, img.tscale + (i << lgh), lgh);
        }
    }
}
// k_ag_group_f32's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAgGroupMx2dGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp mx2d_check) list of buckets — one fp32 matrix each, in shard blocks — through
// k_ag_group_mxfp8_2d, ALLRED_MX2D_GROUP_MAX buckets per launch in list order.  dry: nothing is launched
// and the number of launches is returned.
int launch_ag_group_mxfp8_2d(const allred_mx2d_bucket_f32* buckets, int count, int total, bool rceil, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Mx2dSide side{};
    auto add = [&](int i, int slot) {
        const allred_mx2d_bucket_f32& b = buckets[i];
        Mx2dShape shape;
        uint64_t units, all;
        // the caller's checks, kept next to their use
        if (total < 8 || b.cols == 0 || b.elems_per_rank % b.cols ||
            !mx2d_shape_make(&shape, b.cols, b.elems_per_rank / b.cols, (uint64_t)total, &units, &all))
            return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);
        side.tab.e[slot] = Mx2dEntry{b.shard, b.shard_stride, b.scales, b.scale_stride, b.t_rows, b.t_row_stride,
                                     b.t_scales, b.t_scale_stride, shape};
        side.rows = side.rows || b.rows != nullptr;
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, all, units});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int, uint64_t) {
        const bool rows = side.rows;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, span, side.tab);
                trace_launch(grid, kBlock, "k_ag_group_mxfp8_2d<%d, %s, %s>", total, tf(rceil), tf(rows));
            };
            if (rceil) rows ? go(k_ag_group_mxfp8_2d<p(), true, true>) : go(k_ag_group_mxfp8_2d<p(), true, false>);
            else rows ? go(k_ag_group_mxfp8_2d<p(), false, true>) : go(k_ag_group_mxfp8_2d<p(), false, false>);
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kMx2dGroupMax>(count, dry, side, add, [](uint64_t units) { return persistent_grid(units, kAgGroupMx2dGrid); },
                                      launch);
}

}  // namespace tsa
