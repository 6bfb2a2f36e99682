// adamw_mx2d_kernels.hip — AdamW on the fp32 shards inside the 2D MXFP8 all-gather launch
// (allred_plan_adamw_all_gather_shards_mxfp8_2d, allred.h): the MXFP8 training step in two launches with
// BOTH GEMM operands — the row-wise rows of Y = X W^T and the column-wise rows of dX = dY W — each rounded
// once from the fp32 p'.
//
//   k_adamw_ag_mxfp8_2d<P, ZERO, RCEIL, ROWS>   the persistent grouped walk (group_span.hpp) over PATCHES of
//                                               whole 32 x 32 squares (mx2d_span.hpp) of the four planes;
//                                               ROWS = false: no bucket of the launch has row-wise rows.
//
// The update is adamw_elem below — the lines k_adamw_ag_groups_f32 runs, restated — with adamw_body.hpp's
// call_wide and per_group, and depends on the build's -ffp-contract=off as adamw_kernels.hip does; the
// quantisation is mx2d_image.hpp's quant8, the one k_ag_group_mxfp8_2d runs.  No inline assembly and no
// hand-written wait here beyond lds_barrier() (device.hpp).
#include <type_traits>

#include "adamw_body.hpp"
#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"
#include "mx2d_image.hpp"
#include "mx2d_span.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

constexpr int kAdamwMx2dGroupMax = ALLRED_ADAMW_MX2D_GROUP_MAX;   // buckets of one launch

// Entry i for bucket i of the launch.  GroupSpan carries the row-wise element rows as in mx2d_kernels.hip:
// GroupBucket::ranks is the bucket's row 0 of BYTES (nullptr: no row-wise outputs), ::stride its row stride
// in BYTES.  120 bytes per entry.
struct AdamwMx2dEntry {
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
    Mx2dShape shape;
};
struct AdamwMx2dTable {
    AdamwMx2dEntry e[kAdamwMx2dGroupMax];   // entries past the last bucket: zero
};
// the parameter group of every bucket of the LAUNCH, as adamw_body.hpp's AdamwGroupOf: four bytes to a word
struct AdamwMx2dGroupOf {
    uint32_t w[kAdamwMx2dGroupMax / 4];     // bytes past the last bucket: zero
};
// GroupSpan 2064 + the table 16 x 120 + the group bytes 16 + three pointers and ngroups 32 = 4032 bytes
constexpr size_t kAdamwMx2dArgs = sizeof(GroupSpan) + sizeof(AdamwMx2dTable) + sizeof(AdamwMx2dGroupOf) + 3 * 8 + 8;
static_assert(sizeof(AdamwMx2dEntry) == 120 && sizeof(AdamwMx2dTable) == 120 * kAdamwMx2dGroupMax, "the kernel-argument layout");
static_assert(sizeof(AdamwMx2dGroupOf) == kAdamwMx2dGroupMax && kAdamwMx2dGroupMax % 4 == 0, "one byte per bucket of a launch");
static_assert(kAdamwMx2dArgs == 4032 && kAdamwMx2dArgs < 4096, "kernel arguments stay below 4 KiB");
static_assert(kAdamwMx2dArgs + sizeof(AdamwMx2dEntry) + 1 >= 4096, "ALLRED_ADAMW_MX2D_GROUP_MAX is the largest count that fits");
static_assert(kAdamwMx2dGroupMax <= kGroupMax, "GroupSpan's table holds a launch");
static_assert(sizeof(allred_adamw_mx2d_bucket_f32) == 120, "allred.h's layout");

// allred.h's update of ONE element with a set's values and the call's c.  RESTATED from adamw_body.hpp's
// `update` (the six lines of its loop, in its order, one fp32 operation per operator, never an fma), not
// shared with it: with the lines moved into a function of that header the compiler scheduled every
// k_adamw_ag_* instance differently (profiles/adamw_mx2d_isa_shared_update.txt), and this file changes no existing
// code.  What keeps the two copies from drifting apart is tests/test_gpu_adamw_mx2d.py's GPU-against-GPU guarantee:
// the planes this kernel leaves are bit for bit those of k_adamw_ag_groups_f32.
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

// the launcher's side table: the kernel's tables and whether a member of the pending launch has row-wise rows
struct AdamwMx2dSide {
    AdamwMx2dTable tab;
    AdamwMx2dGroupOf groups;
    bool rows;
};

// ---------------------------------------------------------------------------
// k_adamw_ag_mxfp8_2d<P, ZERO, RCEIL, ROWS>: k_ag_group_mxfp8_2d's walk — a persistent grid, workgroup g
// takes units g + j * G through a forward-only wave-uniform cursor over GroupSpan; a unit is a patch of
// sh x sw squares of one shard block (mx2d_unit_at, unchanged: `src` is the offset into all four planes),
// taken square by square — with the planes REWRITTEN.
// WHO TOUCHES THE PLANES.  adamw_ag lets wave 0 alone touch them, because its four waves would load the
// same kilobyte.  Here a square is 1024 floats and thread tid owns four of them: floats 4 c .. 4 c + 3
// (c = tid & 7) of row r = tid >> 3.  All 256 threads load p, g, m, v with four 16-byte loads, run
// adamw_elem on their four elements and store p', m', v' (ZERO: and +0 over g) to exactly the elements they
// loaded.  Squares of a patch, patches of a block, blocks of a bucket and the buckets' plane blocks
// (engine.cpp adamw_mx2d_check) are pairwise disjoint and every unit is taken by ONE workgroup, so no
// element of the grid is read or written by two threads: nobody can load a p' for a p.
// PREFETCH.  The next square's four loads (the next unit's first square, at a patch's end) are issued before
// this square's arithmetic, into registers of their own.  They read elements no thread has stored to.  A
// workgroup's LAST square is peeled: it has no loads behind it, where k_ag_group_mxfp8_2d reads its last
// unit's first square once more — a square whose planes may be rewritten by then.
// CALL-WIDE AND PER-GROUP VALUES.  Every wave runs adamw_body.hpp's prologue for itself: lane g loads
// hyper[g] (lanes >= ngroups the last set again), call_wide runs on norm_sq, lane g forms per_group.
// call_wide is a fixed order of fp32 operations inside one wave, so the four waves hold the same bits
// without an LDS hand-off.  Per unit the bucket's group comes from the by-value byte table through the
// wave-uniform cursor, and the eight values are read out of lane `group` with v_readlane_b32.  Thread 0 of
// workgroup 0 stores info = {N, c, skip, +0}; the host passes info to the call's FIRST launch alone.
// PER SQUARE, x = p' (skip, N non-finite: p; then nothing is stored to param, exp_avg, exp_avg_sq):
//   row-wise     the thread's four x are a quarter of a row block of eight aligned lanes: quant8; the dword
//                of bytes goes to the image's `rows`, lane c = 0's scale byte to `rscale`.
//   the floats   x goes to F[n & 1], 32 rows of kFStride floats, n the squares this workgroup has staged;
//   barrier;
//   column-wise  thread tid reads rows 4 c .. 4 c + 3 of column r of F[n & 1]: quant8 again; the dword goes
//                to `t`, lane c = 0's byte to `tscale`.
//   the planes   p' m' v' and the +0 are stored BEHIND the barrier and behind the square's LDS work: in
//                front of it the compiler holds a wave at the barrier until the stores have read their data
//                registers (adamw_body.hpp), and every wave of the workgroup waits with it.
// Behind the patch's last square: barrier; every wave streams BOTH element images, 16 bytes per lane, with
// nontemporal stores to its P / 4 rank rows and t rows, and the scale images with plain stores.
// LDS hazards: mx2d_kernels.hip's argument, unchanged — F[n & 1] is written in front of square n's barrier,
// read behind it and written again at square n + 2, behind the barrier of square n + 1 that no wave passes
// before every wave has done its reads of square n; image[j & 1] is written during unit j, read behind
// unit j's last barrier and written again during unit j + 2, behind the barriers of unit j + 1.  The
// hyperparameters never pass through LDS.
// ---------------------------------------------------------------------------
template <int P, bool ZERO, bool RCEIL, bool ROWS>
__global__ __launch_bounds__(kBlock) void k_adamw_ag_mxfp8_2d(GroupSpan span, AdamwMx2dTable tab, AdamwMx2dGroupOf group_of,
                                                              const allred_adamw_hyper* __restrict__ hyper, int ngroups,
                                                              const float* __restrict__ norm_sq, float* info) {
    constexpr int RPW = P / 4;
    constexpr uint32_t LGP = P == 8 ? 3 : P == 16 ? 4 : P == 32 ? 5 : 6;
    static_assert((1 << LGP) == P, "P = 8, 16, 32 or 64");
    __shared__ Mx2dImage image[2];
    __shared__ __attribute__((aligned(16))) float F[2][32 * kFStride];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = tid >> 3, c = tid & 7;
    // Copies, not pointers into the by-value tables: those stay in the kernel-argument segment.  A Unit holds what
    // the squares need — the planes, the patch's shape, its offset into the planes.  The outputs' pointers, strides
    // and offsets are formed behind the unit's last square from the tables again (`bucket`, `block`, `rem`): held
    // across the squares they took the scalar registers that the hyperparameters need, and 10 to 12 of them spilled.
    struct Unit {
        float* param;
        float* grad;
        float* exp_avg;
        float* exp_avg_sq;
        uint64_t cols;
        uint32_t lgh, lgw;
        uint64_t src;      // mx2d_unit_at's
        uint32_t bucket;   // index within the LAUNCH
        uint32_t block, rem;
        uint32_t group;    // the bucket's parameter group
        bool rows;         // the bucket has row-wise outputs
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const AdamwMx2dEntry& e = tab.e[gt.bucket];
        const uint32_t word = group_of.w[(gt.bucket >> 2) & (kAdamwMx2dGroupMax / 4 - 1)];
        return Unit{e.param,
                    e.grad,
                    e.exp_avg,
                    e.exp_avg_sq,
                    e.shape.cols,
                    e.shape.lgh,
                    e.shape.lgw,
                    mx2d_unit_at(e.shape, gt.block, gt.rem, e.shard_stride, LGP).src,
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
    // square q of the unit is (q >> lgw, q & (sw - 1)) in (row, column) squares; the thread's four floats of it
    auto at = [&](const Unit& u, uint32_t q) {
        const uint64_t i = ((uint64_t)(q >> u.lgw) << 5) + (uint32_t)r, j = ((uint64_t)(q & ((1u << u.lgw) - 1)) << 5) + 4u * (uint32_t)c;
        return u.src + i * u.cols + j;
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
        const uint32_t lgh = cu.lgh, lgw = cu.lgw, squares = 1u << (lgh + lgw);
        Mx2dImage& img = image[j & 1];
        const bool rows = ROWS && cu.rows;               // uniform over the workgroup
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
                const Quant a = quant8<RCEIL>(p);
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
            // the planes: the elements this thread loaded, and no other
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
        const AdamwMx2dEntry& oe = tab.e[cu.bucket];
        const Mx2dUnit out = mx2d_unit_at(oe.shape, cu.block, cu.rem, oe.shard_stride, LGP);
        const uint64_t cols = oe.shape.cols, nrows = oe.shape.nrows;
        for (uint32_t i = 0; i < squares; ++i) {
            const uint32_t o = i * 1024 + 16 * (uint32_t)lane;
            if (rows) {
                const u32x4 e = *reinterpret_cast<const u32x4*>(img.rows + o);
                uint8_t* d = reinterpret_cast<uint8_t*>(ob.ranks) + out.row + (uint64_t)(o >> (5 + lgw)) * cols + (o & ((32u << lgw) - 1));
#pragma unroll
                for (int k = 0; k < RPW; ++k)
                    __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(d + (uint64_t)(RPW * w + k) * ob.stride));
            }
            const u32x4 e = *reinterpret_cast<const u32x4*>(img.t + o);
            uint8_t* d = oe.t_rows + out.t + (uint64_t)(o >> (5 + lgh)) * nrows + (o & ((32u << lgh) - 1));
#pragma unroll
            for (int k = 0; k < RPW; ++k)
                __builtin_nontemporal_store(e, reinterpret_cast<u32x4*>(d + (uint64_t)(RPW * w + k) * oe.t_row_stride));
        }
        // the scale bytes: row i's sw bytes, column j's sh bytes; NOT nontemporal (k_ag_group_mxfp8's finding)
        if (rows) {
            for (uint32_t i = (uint32_t)lane; i < (32u << lgh); i += 64) {
                uint8_t* d = oe.scales + out.rscale + (uint64_t)i * (cols >> 5);
                for (int k = 0; k < RPW; ++k) put_scales(d + (uint64_t)(RPW * w + k) * oe.scale_stride, img.rscale + (i << lgw), lgw);
            }
        }
        for (uint32_t i = (uint32_t)lane; i < (32u << lgw); i += 64) {
            uint8_t* d = oe.t_scales + out.tscale + (uint64_t)i * (nrows >> 5);
            for (int k = 0; k < RPW; ++k) put_scales(d + (uint64_t)(RPW * w + k) * oe.t_scale_stride, img.tscale + (i << lgh), lgh);
        }
    }
}
// k_ag_group_f32's grid cap, inherited and unmeasured here (tune pipe_grid caps it lower)
constexpr uint64_t kAdamwMx2dGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp adamw_mx2d_check) list of buckets — one fp32 matrix each as four planes in shard
// blocks — through k_adamw_ag_mxfp8_2d, ALLRED_ADAMW_MX2D_GROUP_MAX buckets per launch in list order whatever
// the groups are.  hyper is ngroups >= 1 sets and group_of the buckets' groups (nullptr: every bucket in group
// 0); a launch's group table is indexed by the bucket's place in the LAUNCH.  info goes to the first launch
// alone: it is written once.  dry: nothing is launched and the number of launches is returned.
int launch_adamw_group_mxfp8_2d(const allred_adamw_mx2d_bucket_f32* buckets, const uint8_t* group_of, int count, int total,
                                const allred_adamw_hyper* hyper, int ngroups, const float* norm_sq, float* info, bool zero_grad,
                                bool rceil, bool dry, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    AdamwMx2dSide side{};
    if (ngroups < 1 || ngroups > kParamGroupsMax) return ALLRED_ERR_ARG;   // the caller's check, kept next to its use
    auto add = [&](int i, int slot) {
        const allred_adamw_mx2d_bucket_f32& b = buckets[i];
        Mx2dShape shape;
        uint64_t units, all;
        const uint32_t g = group_of ? group_of[i] : 0u;
        // the caller's checks, kept next to their use
        if (total < 8 || b.cols == 0 || b.elems_per_rank % b.cols ||
            !mx2d_shape_make(&shape, b.cols, b.elems_per_rank / b.cols, (uint64_t)total, &units, &all))
            return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);
        if (g >= (uint32_t)ngroups) return BatchAdd::error(ALLRED_ERR_ARG);
        side.tab.e[slot] = AdamwMx2dEntry{b.param,  b.grad,         b.exp_avg,  b.exp_avg_sq,     b.shard_stride, b.scales, b.scale_stride,
                                          b.t_rows, b.t_row_stride, b.t_scales, b.t_scale_stride, shape};
        side.groups.w[slot >> 2] |= g << (8 * (slot & 3));
        side.rows = side.rows || b.rows != nullptr;
        return BatchAdd::member(GroupIn{reinterpret_cast<uint16_t*>(b.rows), b.row_stride, all, units});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t) {
        const bool rows = side.rows;
        float* out = index == 0 ? info : nullptr;
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            auto go = [&](auto zero, auto rc, auto rw) {
                hipLaunchKernelGGL((k_adamw_ag_mxfp8_2d<p(), decltype(zero)::value, decltype(rc)::value, decltype(rw)::value>), dim3(grid),
                                   dim3(kBlock), 0, st, span, side.tab, side.groups, hyper, ngroups, norm_sq, out);
                trace_launch(grid, kBlock, "k_adamw_ag_mxfp8_2d<%d, %s, %s, %s>", total, tf(zero_grad), tf(rceil), tf(rows));
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
    return group_batch<kAdamwMx2dGroupMax>(count, dry, side, add, [](uint64_t units) { return persistent_grid(units, kAdamwMx2dGrid); },
                                           launch);
}

}  // namespace tsa
