// adamw_mx4_2d_kernels.hip — AdamW on the fp32 shards inside the 2D MXFP4 all-gather launch
// (allred_plan_adamw_all_gather_shards_mxfp4_2d, allred.h): the MXFP4 training step in two launches with
// BOTH GEMM operands — the row-wise nibble rows of Y = X W^T and the column-wise rows of dX = dY W — each
// rounded once from the fp32 p', in the register it is computed in.
//
//   k_adamw_ag_mxfp4_2d<P, ZERO, RCEIL, ROWS>   the persistent grouped walk (group_span.hpp) over STRIPS of
//                                               the matrix (mx4_2d_span.hpp, unchanged): S consecutive 32-row
//                                               groups of the four planes, taken from as many neighbouring
//                                               shard blocks as they lie in, by up to 128 columns;
//                                               ROWS = false: no bucket of the launch has row-wise rows.
//
// It is k_ag_group_mxfp4_2d's strip walk (mx4_2d_kernels.hip) with the planes REWRITTEN, not
// k_adamw_ag_mxfp8_2d (adamw_mx2d_kernels.hip) with another converter: a patch of that kernel lies in one
// shard block, a strip's row groups may each lie in another, so the offset into the planes is formed per
// SQUARE.  The update is adamw_elem below — the lines k_adamw_ag_groups_f32 runs, restated — with
// adamw_body.hpp's call_wide and per_group, and depends on the build's -ffp-contract=off as adamw_kernels.hip
// does; the quantisation is quant8_fp4 below, k_ag_group_mxfp4_2d's restated.  No inline assembly and no
// hand-written wait here beyond lds_barrier() (device.hpp).
#include <type_traits>

#include "adamw_body.hpp"
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx2d_image.hpp"
#include "mx4_2d_span.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

constexpr int kAdamwMx4GroupMax = ALLRED_ADAMW_MX4_2D_GROUP_MAX;   // buckets of one launch
constexpr int kS = 1 << kMx4LgStrip;                               // row groups of a strip
constexpr int kStripSquares = 1 << kMx4LgSquares;                  // 32 x 32 squares of the largest strip

// Entry i for bucket i of the launch.  GroupSpan carries the row-wise element rows as in mx4_2d_kernels.hip:
// GroupBucket::ranks is the bucket's row 0 of BYTES (nullptr: no row-wise outputs), ::stride its row stride
// in BYTES.  120 bytes per entry.
struct AdamwMx4Entry {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t shard_stride;     // floats, ONE stride for the four planes
    uint8_t* scales;
    uint64_t scale_stride;     // bytes
    uint8_t* t_rows;
    uint64_t t_row_stride;     // bytes
    uint8_t* t_scales;
    uint64_t t_scale_stride;   // bytes
    Mx4Shape shape;
};
struct AdamwMx4Table {
    AdamwMx4Entry e[kAdamwMx4GroupMax];   // entries past the last bucket: zero
};
// the parameter group of every bucket of the LAUNCH, as adamw_body.hpp's AdamwGroupOf: four bytes to a word
struct AdamwMx4GroupOf {
    uint32_t w[kAdamwMx4GroupMax / 4];    // bytes past the last bucket: zero
};
// GroupSpan 2064 + the table 16 x 120 + the group bytes 16 + three pointers and ngroups 32 = 4032 bytes
constexpr size_t kAdamwMx4Args = sizeof(GroupSpan) + sizeof(AdamwMx4Table) + sizeof(AdamwMx4GroupOf) + 3 * 8 + 8;
static_assert(sizeof(AdamwMx4Entry) == 120 && sizeof(AdamwMx4Table) == 120 * kAdamwMx4GroupMax, "the kernel-argument layout");
static_assert(sizeof(AdamwMx4GroupOf) == kAdamwMx4GroupMax && kAdamwMx4GroupMax % 4 == 0, "one byte per bucket of a launch");
static_assert(kAdamwMx4Args == 4032 && kAdamwMx4Args < 4096, "kernel arguments stay below 4 KiB");
static_assert(kAdamwMx4Args + sizeof(AdamwMx4Entry) + 1 >= 4096, "ALLRED_ADAMW_MX4_2D_GROUP_MAX is the largest count that fits");
static_assert(kAdamwMx4GroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_adamw_mx2d_bucket_f32) == 120, "allred.h's layout");

// allred.h's update of ONE element with a set's values and the call's c.  RESTATED from adamw_body.hpp's
// `update` (the six lines of its loop, in its order, one fp32 operation per operator, never an fma), as
// adamw_mx2d_kernels.hip restates them and for its reason: with the lines moved into a function of that
// header the compiler scheduled every k_adamw_ag_* instance differently
// (profiles/adamw_mx2d_isa_shared_update.txt), and this file changes no existing code.  What keeps the copies
// from drifting apart is tests/test_gpu_adamw_mx4_2d.py's GPU-against-GPU guarantee: the planes this kernel
// leaves are bit for bit those of k_adamw_ag_groups_f32.
struct AdamwElem {
    float p, m, v;
};
__device__ __forceinline__ AdamwElem adamw_elem(float p, float g, float m, float v, float c, const PerGroup& s) {
    AdamwElem y;
    const float g1 = g * c;
    const float p1 = p * s.d;
    y.m = m * s.beta1 + g1 * s.o1;
    y.v = v * s.beta2 + (g1 * g1) * s.o2;
    const float den = sqrtf(y.v) / s.bc2 + s.eps;
    y.p = p1 - s.ss * (y.m / den);
    return y;
}

// One strip's quantised nibbles as they leave: both element images and both scale images, plain linear.
// 512 bytes of each element image per square.  RESTATED from mx4_2d_kernels.hip, which keeps its copy in its
// anonymous namespace: that file is not touched, so k_ag_group_mxfp4_2d's code cannot change.  The guarantee
// test compares the two quantisers bit for bit.
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

// allred.h's MXFP4 rule for 32 consecutive floats held as four per lane by EIGHT aligned lanes: three DPP
// steps for the integer amax, then k_ag_group_mxfp4's arithmetic unchanged.  BOTH directions of a square go
// through it: a row block of p' before the transpose, a column block behind it.
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

// the launcher's side table: the kernel's tables and whether a member of the pending launch has row-wise rows
struct AdamwMx4Side {
    AdamwMx4Table tab;
    AdamwMx4GroupOf groups;
    bool rows;
};

// ---------------------------------------------------------------------------
// k_adamw_ag_mxfp4_2d<P, ZERO, RCEIL, ROWS>: a persistent grid, workgroup g takes units g + j * G through a
// forward-only wave-uniform cursor over GroupSpan.  A unit is a strip of S x sw squares of the MATRIX
// (mx4_2d_unit_at: GroupTile.block is the strip, .rem the column group), taken square by square, square q at
// row group g0 + (q >> lgw) of the matrix and column square q & (sw - 1) of the unit.
// PLANE OFFSETS PER SQUARE.  Every row group of a strip may lie in another shard block: `at` forms the
// offset of the thread's four floats from mx4_2d_group_at(shape, g0 + (q >> lgw), shard_stride) — one
// multiply by the host's reciprocal and one correction, wave-uniform — for every square.  There is ONE
// shard_stride for the four planes, and `at` with the same (unit, q) serves the four loads and the three or
// four stores of a square: a thread stores exactly where it loaded.
// WHO TOUCHES THE PLANES.  Thread tid owns floats 4 c .. 4 c + 3 (c = tid & 7) of row r = tid >> 3 of each
// square.  All 256 threads load p, g, m, v with four 16-byte loads, run adamw_elem on their four elements and
// store p', m', v' (ZERO: and +0 over g) to exactly the elements they loaded.  Squares of a strip, strips of a
// matrix, the shard blocks they lie in and the buckets' plane blocks (engine.cpp adamw_mx2d_check) are
// pairwise disjoint and every unit is taken by ONE workgroup, so no element of the grid is read or written by
// two threads: nobody can load a p' for a p.
// PREFETCH.  The next square's four loads (the next unit's first square, at a strip's end) are issued before
// this square's arithmetic, into registers of their own.  They read elements no thread has stored to.  A
// workgroup's LAST square is peeled: it has no loads behind it, where k_ag_group_mxfp4_2d reads its last
// unit's first square once more — a square whose planes hold p' by then (and, with ZERO, +0 for g).
// CALL-WIDE AND PER-GROUP VALUES.  As k_adamw_ag_mxfp8_2d: every wave runs adamw_body.hpp's prologue for
// itself — lane g loads hyper[g] (lanes >= ngroups the last set again), call_wide runs on norm_sq, lane g
// forms per_group; call_wide is a fixed order of fp32 operations inside one wave, so the four waves hold the
// same bits without an LDS hand-off.  Per unit the bucket's group comes from the by-value byte table through
// the wave-uniform cursor, and the eight values are read out of lane `group` with v_readlane_b32.  Thread 0
// of workgroup 0 stores info = {N, c, skip, +0}; the host passes info to the call's FIRST launch alone.
// PER SQUARE, x = p' (skip, N non-finite: p; then nothing is stored to param, exp_avg, exp_avg_sq):
//   row-wise     the thread's four x are a quarter of a row block of eight aligned lanes: quant8_fp4; its
//                four nibbles are TWO WHOLE BYTES of the image's `rows` — one 2-byte LDS store, no byte
//                shared between threads —, lane c = 0's scale byte goes to `rscale`;
//   the floats   x goes to F[n & 1], 32 rows of kFStride floats, n the squares this workgroup has staged;
//   barrier;
//   column-wise  thread tid reads rows 4 c .. 4 c + 3 of column r of F[n & 1], four CONSECUTIVE elements of
//                the t row: quant8_fp4 again, two whole bytes to `t`, lane c = 0's scale byte to `tscale`;
//   the planes   p' m' v' and the +0 are stored BEHIND the barrier and behind the square's LDS work: in
//                front of it the compiler holds a wave at the barrier until the stores have read their data
//                registers (adamw_body.hpp), and every wave of the workgroup waits with it.
// Behind the strip's last square: barrier; the outputs' pointers, strides and offsets are formed from the
// by-value tables again; every wave streams BOTH nibble images, 16 bytes per lane and 1 KiB per instruction,
// with nontemporal stores to its P / 4 rank rows and t rows — runs of 16 sw bytes in a row, of 16 S bytes in
// a t row —, and the scale images with plain stores of sw or S bytes, exactly as k_ag_group_mxfp4_2d does.
// LDS HAZARDS.  F[n & 1] is written in front of square n's barrier, read behind it and written again at
// square n + 2; between a wave's read at square n and any wave's write at square n + 2 lies the barrier of
// square n + 1, which no wave passes before every wave has arrived, i.e. has done its reads of square n.  n
// counts across units, and behind a strip's last square lies one more barrier, so the argument holds across a
// strip's end too.  image[j & 1] is written during unit j (the row-wise bytes in front of a square's barrier,
// the t bytes behind it), read behind unit j's last barrier — the one behind its last square, which every
// wave reaches only behind its last t bytes — and written again during unit j + 2, after the S sw >= 4
// barriers of unit j + 1, which every wave reaches only behind its reads of unit j.  Inside an image no byte
// has two writers: a thread's four nibbles are bytes 2 c and 2 c + 1 of its row's (column's) 16 bytes of the
// square.  The plane stores touch no LDS, and the hyperparameters never pass through it.
// ---------------------------------------------------------------------------
template <int P, bool ZERO, bool RCEIL, bool ROWS>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_mxfp4_2d(GroupSpan span, AdamwMx4Table tab, AdamwMx4GroupOf group_of,
                                                              const allred_adamw_hyper* __restrict__ hyper, int ngroups,
                                                              const float* __restrict__ norm_sq, float* info) {
    constexpr int RPW = P / 4;
    constexpr uint32_t LGT = 4 + kMx4LgStrip;   // bytes of a column of the t image, as a shift: 16 S
    static_assert(P == 8 || P == 16 || P == 32 || P == 64, "P = 8, 16, 32 or 64");
    __shared__ Mx4Image image[2];
    __shared__ __attribute__((aligned(16))) float F[2][32 * kFStride];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = tid >> 3, c = tid & 7;
    // Copies, not pointers into the by-value tables: those stay in the kernel-argument segment.  A Unit holds what
    // the squares need — the planes, their stride, the matrix's shape, the strip's first row group and column.  The
    // outputs' pointers, strides and offsets are formed behind the unit's last square from the tables again
    // (`bucket`, `strip`, `cg`): held across the squares they took 10 to 12 scalar registers too many in
    // k_adamw_ag_mxfp8_2d, and spilled.
    struct Unit {
        float* param;
        float* grad;
        float* exp_avg;
        float* exp_avg_sq;
        uint64_t shard_stride;
        Mx4Shape shape;
        uint64_t j0;        // mx4_2d_unit_at's: the strip's first column
        uint32_t g0;        // and its first row group of the matrix
        uint32_t bucket;    // index within the LAUNCH
        uint32_t strip, cg;
        uint32_t group;     // the bucket's parameter group
        bool rows;          // the bucket has row-wise outputs
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const AdamwMx4Entry& e = tab.e[gt.bucket];
        const uint32_t word = group_of.w[(gt.bucket >> 2) & (kAdamwMx4GroupMax / 4 - 1)];
        const Mx4Unit at = mx4_2d_unit_at(e.shape, gt.block, gt.rem);
        return Unit{e.param,
                    e.grad,
                    e.exp_avg,
                    e.exp_avg_sq,
                    e.shard_stride,
                    e.shape,
                    at.j0,
                    at.g0,
                    gt.bucket,
                    gt.block,
                    gt.rem,
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)((word >> (8 * (gt.bucket & 3))) & 0xFF)),
                    span.b[gt.bucket].ranks != nullptr};
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    if (mine <= 0) return;   // the whole workgroup: no barrier is left waiting
    const int last = mine - 1;
    struct Src {
        f32x4 p, g, m, v;
    };
    // the thread's four floats of square q of the unit, as an offset into ALL FOUR planes: the row group's shard
    // block per square (wave-uniform), the thread's row and column inside it
    auto at = [&](const Unit& u, uint32_t q) {
        const Mx4Group g = mx4_2d_group_at(u.shape, u.g0 + (q >> u.shape.lgw), u.shard_stride);
        const uint64_t j = u.j0 + ((uint64_t)(q & ((1u << u.shape.lgw) - 1)) << 5) + 4u * (uint32_t)c;
        return g.src + (uint64_t)r * u.shape.cols + j;
    };
    auto load = [&](const Unit& u, uint32_t q) {
        const uint64_t i = at(u, q);
        return Src{*reinterpret_cast<const f32x4*>(u.param + i), *reinterpret_cast<const f32x4*>(u.grad + i),
                   *reinterpret_cast<const f32x4*>(u.exp_avg + i), *reinterpret_cast<const f32x4*>(u.exp_avg_sq + i)};
    };
    // every wave: the reads of hyper (lane g reads group g; lanes >= ngroups the LAST set again, never past
    // the array) and norm_sq go out first, the first square's loads behind them, then the uniform arithmetic
    const f32x4* hp = reinterpret_cast<const f32x4*>(hyper + (lane < ngroups ? lane : ngroups - 1));
    const f32x4 h0 = hp[0], h1 = hp[1];
    float nsq = 0.0f;
    if (norm_sq && lane < P) nsq = norm_sq[lane];
    Src x = load(locate(0), 0);
    allred_adamw_hyper h;
    h.lr = h0[0];
    h.beta1 = h0[1];
    h.beta2 = h0[2];
    h.eps = h0[3];
    h.weight_decay = h1[0];
    h.bias_corr1 = h1[1];
    h.bias_corr2_sqrt = h1[2];
    h.max_norm = h1[3];
    const CallWide u = call_wide(from_lane(h.max_norm, 0), nsq, norm_sq != nullptr);
    const PerGroup lanes = per_group(h);
    if (info && blockIdx.x == 0 && tid == 0) *reinterpret_cast<f32x4*>(info) = f32x4{u.N, u.c, u.skip ? 1.0f : 0.0f, 0.0f};
    // the same in every lane (call_wide): as scalars
    const float clip = from_lane(u.c, 0);
    const bool skip = __builtin_amdgcn_readfirstlane((int)u.skip) != 0;
    uint32_t staged = 0;
    for (int j = 0; j < mine; ++j) {
        // located again, not carried over from the prefetch below: a Unit that lives across iterations ends up in
        // scratch, and the second walk of the same unit is scalar work (the cursor stands still for it)
        const Unit cu = locate(j);
        const uint32_t lgw = cu.shape.lgw, squares = (uint32_t)kS << lgw;
        Mx4Image& img = image[j & 1];
        const bool rows = ROWS && cu.rows;              // uniform over the workgroup
        const int g = (int)cu.group;                    // < ngroups <= 8 (the host's check): a lane that holds a loaded set
        const PerGroup s{from_lane(lanes.d, g),     from_lane(lanes.o1, g),    from_lane(lanes.o2, g),  from_lane(lanes.ss, g),
                         from_lane(lanes.beta1, g), from_lane(lanes.beta2, g), from_lane(lanes.eps, g), from_lane(lanes.bc2, g)};
        // One square.  NEXT: a square follows it in this workgroup — its loads go out before this square's arithmetic.
        auto square = [&](uint32_t q, auto next) {
            constexpr bool NEXT = decltype(next)::value;
            Src nx{};
            if constexpr (NEXT) {
                if (q + 1 < squares) {
                    nx = load(cu, q + 1);
                } else {
                    nx = load(locate(j + 1), 0);   // j < last: the last unit's last square is not NEXT
                }
            }
            f32x4 p = x.p, m = x.m, v = x.v;
            if (!skip) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const AdamwElem n = adamw_elem(x.p[e], x.g[e], x.m[e], x.v[e], clip, s);
                    p[e] = n.p;
                    m[e] = n.m;
                    v[e] = n.v;
                }
            }
            const uint32_t qi = q >> lgw, qj = q & ((1u << lgw) - 1);
            float* f = F[staged & 1];
            ++staged;
            *reinterpret_cast<f32x4*>(f + r * kFStride + 4 * c) = p;
            if (rows) {
                const Quant4 a = quant8_fp4<RCEIL>(p);
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
            // the planes: the elements this thread loaded — the same `at` —, and no other
            const uint64_t i = at(cu, q);
            if (!skip) {
                *reinterpret_cast<f32x4*>(cu.param + i) = p;
                *reinterpret_cast<f32x4*>(cu.exp_avg + i) = m;
                *reinterpret_cast<f32x4*>(cu.exp_avg_sq + i) = v;
            }
            if constexpr (ZERO) *reinterpret_cast<f32x4*>(cu.grad + i) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (NEXT) x = nx;
        };
        const uint32_t followed = j < last ? squares : squares - 1;   // squares with a square of this workgroup behind them
        for (uint32_t q = 0; q < followed; ++q) square(q, std::true_type{});
        if (j == last) square(squares - 1, std::false_type{});
        lds_barrier();
        const GroupBucket& ob = span.b[cu.bucket];      // the outputs: read here, not carried across the squares
        const AdamwMx4Entry& oe = tab.e[cu.bucket];
        const Mx4Unit out = mx4_2d_unit_at(oe.shape, cu.strip, cu.cg);
        const uint64_t cols = oe.shape.cols, nrows = oe.shape.nrows;
        // 512 bytes of each image per square, 1 KiB per instruction: squares / 2 trips (squares >= S is even)
        for (uint32_t i = 0; i < squares / 2; ++i) {
            const uint32_t o = i * 1024 + 16 * (uint32_t)lane;
            if (rows) {
                const u32x4 e = *reinterpret_cast<const u32x4*>(img.rows + o);
                uint8_t* d = reinterpret_cast<uint8_t*>(ob.ranks) + out.row + (uint64_t)(o >> (4 + lgw)) * (cols >> 1) + (o & ((16u << lgw) - 1));
#pragma unroll
                for (int k = 0; k < RPW; ++k)
                    __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(d + (uint64_t)(RPW * w + k) * ob.stride));
            }
            const u32x4 e = *reinterpret_cast<const u32x4*>(img.t + o);
            uint8_t* d = oe.t_rows + out.t + (uint64_t)(o >> LGT) * (nrows >> 1) + (o & ((1u << LGT) - 1));
#pragma unroll
            for (int k = 0; k < RPW; ++k)
                __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(d + (uint64_t)(RPW * w + k) * oe.t_row_stride));
        }
        // the scale bytes: row i's sw bytes, column j's S bytes; NOT nontemporal (k_ag_group_mxfp8's finding)
        if (rows) {
            for (uint32_t i = (uint32_t)lane; i < 32u * kS; i += 64) {
                uint8_t* d = oe.scales + out.rscale + (uint64_t)i * (cols >> 5);
                for (int k = 0; k < RPW; ++k) put_scales(d + (uint64_t)(RPW * w + k) * oe.scale_stride, img.rscale + (i << lgw), lgw);
            }
        }
        using StripScales = std::conditional_t<kS == 4, uint32_t, uint64_t>;   // a column's S scale bytes, ONE store
        for (uint32_t i = (uint32_t)lane; i < (32u << lgw); i += 64) {
            uint8_t* d = oe.t_scales + out.tscale + (uint64_t)i * (nrows >> 5);
            const StripScales e = *reinterpret_cast<const StripScales*>(img.tscale + (i << kMx4LgStrip));
            for (int k = 0; k < RPW; ++k) *reinterpret_cast<StripScales*>(d + (uint64_t)(RPW * w + k) * oe.t_scale_stride) = e;
        }
    }
}
// k_ag_group_f32's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwMx4_2dGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp adamw_mx2d_check with the MXFP4 payload) list of buckets — one fp32 matrix each as
// four planes in shard blocks — through k_adamw_ag_mxfp4_2d, ALLRED_ADAMW_MX4_2D_GROUP_MAX buckets per launch
// in list order whatever the groups are.  hyper is ngroups >= 1 sets and group_of the buckets' groups
// (nullptr: every bucket in group 0); a launch's group table is indexed by the bucket's place in the LAUNCH.
// info goes to the first launch alone: it is written once.  dry: nothing is launched and the number of
// launches is returned.
int launch_adamw_group_mxfp4_2d(const allred_adamw_mx2d_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                                const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                                bool rceil, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AdamwMx4Side side{};
    if (ngroups < 1 || ngroups > kParamGroupsMax) return ALLRED_ERR_ARG;   // the caller's check, kept next to its use
    auto add = [&](int i, int slot) {
        const allred_adamw_mx2d_bucket_f32& b = buckets[i];
        Mx4Shape shape;
        uint64_t cgs, all;
        const uint32_t g = group_of ? group_of[i] : 0u;
        // the caller's checks, kept next to their use
        if (total < 8 || b.cols == 0 || b.elems_per_rank % b.cols ||
            !mx4_2d_shape_make(&shape, b.cols, b.elems_per_rank / b.cols, (uint64_t)total, &cgs, &all))
            return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);
        if (g >= (uint32_t)ngroups) return BatchAdd::error(ALLRED_ERR_ARG);
        side.tab.e[slot] = AdamwMx4Entry{b.param,  b.grad,         b.exp_avg,  b.exp_avg_sq,     b.shard_stride, b.scales, b.scale_stride,
                                         b.t_rows, b.t_row_stride, b.t_scales, b.t_scale_stride, shape};
        side.groups.w[slot >> 2] |= g << (8 * (slot & 3));
        side.rows = side.rows || b.rows != nullptr;
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, all, cgs});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t) {
        const bool rows = side.rows;
        float* out = index == 0 ? info : nullptr;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto zero, auto rc, auto rw) {
                hipLaunchKernelGGL((k_adamw_ag_mxfp4_2d<p(), decltype(zero)::value, decltype(rc)::value, decltype(rw)::value>), dim3(grid),
                                   dim3(kBlock), 0, st, span, side.tab, side.groups, hyper, ngroups, norm_sq, out);
                trace_launch(grid, kBlock, "k_adamw_ag_mxfp4_2d<%d, %s, %s, %s>", total, tf(zero_grad), tf(rceil), tf(rows));
            };
            auto with_rows = [&](auto zero, auto rc) {
                if (rows) go(zero, rc, std::true_type{});
                else go(zero, rc, std::false_type{});
            };
            if (zero_grad) {
                if (rceil) with_rows(std::true_type{}, std::true_type{});
                else with_rows(std::true_type{}, std::false_type{});
            } else {
                if (rceil) with_rows(std::false_type{}, std::true_type{});
                else with_rows(std::false_type{}, std::false_type{});
            }
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    return group_batch<kAdamwMx4GroupMax>(count, dry, side, add, [](uint64_t units) { return persistent_grid(units, kAdamwMx4_2dGrid); },
                                          launch);
}

}  // namespace tsa
