// shard_f32_kernels.hip — the grouped shard calls on fp32 SHARDS
// (allred_plan_reduce_scatter_shards_f32 / allred_plan_all_gather_shards_f32,
// allred.h): the two halves of a sharded training step whose gradient shards
// and master parameters are fp32, without the cast passes around them.
//
//   k_tree_group_f32<P, ACC>   k_tree_group's walk; the BO tree of every tile
//                              in fp32 with NO intermediate rounding, times
//                              `scale`, stored to (or added into) the fp32
//                              shard block of the tile.
//   k_tree_group_f32_norm<P, ACC>   the same pass, which also leaves the squared
//                              norm of what it stored, per rank, in norm_sq
//                              (allred_plan_reduce_scatter_shards_f32_norm).
//   k_ag_group_f32<P>          k_ag_group's walk; a tile's 256 floats of the
//                              shard rounded ONCE to bf16 (pack_rne) and
//                              written to every rank row.
//
// The arithmetic here depends on the build's -ffp-contract=off (Makefile,
// HIPFLAGS): `old + s * scale` must be one fp32 multiply and one fp32 add, never
// an fma — allred.h states the result as those two operations and the tests
// compare bits.
#include <type_traits>

#include "device.hpp"
#include "group_batch.hpp"
#include "group_span.hpp"
#include "launch_util.hpp"

namespace tsa {
namespace {

typedef __attribute__((address_space(1))) f32x4 global_f32x4;

// The fp32 shard buffers of a grouped launch: entry i for bucket i of the launch, block b of
// the bucket at shard + b * stride floats.  64 x 16 bytes by value next to the order pointer,
// GroupSpan and the scale: 8 + 2064 + 1024 + 4 = 3100 bytes of kernel arguments, inside 4 KiB.
struct GroupShardF32 {     // 16 bytes
    float* shard;
    uint64_t stride;       // floats
};
struct GroupShardsF32 {
    GroupShardF32 s[kGroupMax];   // entries past the last bucket: zero
};
static_assert(sizeof(GroupShardF32) == 16 && sizeof(GroupShardsF32) == 16 * kGroupMax, "the kernel-argument layout");

// What k_tree_group_f32_norm takes on top: two pointers, a tile offset and a launch index.
constexpr uint32_t kNormCounterBytes = 64;   // the arrival counter's block at the head of the workspace
struct NormArgs {          // 24 bytes
    float* norm_sq;        // [P]: launch 0 overwrites it, launch k > 0 adds to what launch k - 1 left
    void* ws;              // kNormCounterBytes (the counter in the first 4), then one float per tile of the call
    uint32_t tile_off;     // tiles of the launches before this one: this launch's region of the partials
    uint32_t launch;       // index of this launch in the call
};
static_assert(sizeof(NormArgs) == 24, "the kernel-argument layout");
static_assert(8 + sizeof(GroupSpan) + sizeof(GroupShardsF32) + 8 + sizeof(NormArgs) < 4096, "kernel arguments stay below 4 KiB");
typedef __attribute__((address_space(1))) uint32_t global_rw_u32;

// How the finalizer of k_tree_group_f32_norm reads the other workgroups' partials — both are valid
// forms of the in-launch hand-off (the partials are written through and drained before the ticket):
//   0  one lane's agent-scope acquire fence before the barrier, then plain vector loads;
//   1  no fence, EVERY load of a partial an agent-scope atomic load (sc1: past this CU's L1).
// A build-time switch for the A/B of DESIGN.md §14, not a tune key; the default is the form measured faster.
#ifndef ALLRED_NORM_SC1_LOADS
#define ALLRED_NORM_SC1_LOADS 0
#endif
constexpr bool kNormSc1Loads = ALLRED_NORM_SC1_LOADS != 0;

// ---------------------------------------------------------------------------
// The BO tree in fp32: tree_levels / tree_wave_part / tree_join4 of device.hpp
// with every node 8 floats instead of 8 bf16 — leaves widened exactly (<< 16),
// every add one IEEE fp32 add, nothing rounded to bf16.  Same pairing, same
// operand order (fp32 addition is commutative in every bit but a NaN's payload).
// ---------------------------------------------------------------------------
struct F8 {
    f32x4 a, b;   // elements 0-3 and 4-7 of a 16-byte bf16 vector
};

__device__ __forceinline__ F8 widen8(uint4 x) {
    F8 r;
    r.a = f32x4{lo_f(x.x), hi_f(x.x), lo_f(x.y), hi_f(x.y)};
    r.b = f32x4{lo_f(x.z), hi_f(x.z), lo_f(x.w), hi_f(x.w)};
    return r;
}

__device__ __forceinline__ F8 add8f(const F8& x, const F8& y) { return F8{x.a + y.a, x.b + y.b}; }

template <int N>
__device__ __forceinline__ void tree_levels_f32(F8 (&x)[N]) {
#pragma unroll
    for (int s = 1; s < N; s *= 2)
#pragma unroll
        for (int i = 0; i < N; i += 2 * s) x[i] = add8f(x[i], x[i + s]);
}

// A wave's share of a tile's tree, as tree_wave_part: this lane's LPL adjacent leaves ord[0 .. LPL)
// of column c widened and summed in registers, then the level across the wave's two lane halves.
template <int TV, int LPL>
__device__ __forceinline__ F8 tree_wave_part_f32(const uint4* tile, const uint8_t* ord, int c) {
    F8 x[LPL];
#pragma unroll
    for (int i = 0; i < LPL; ++i) x[i] = widen8(tile[(int)ord[i] * TV + c]);
    tree_levels_f32(x);
    F8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.a[i] = add_halves(x[0].a[i]);
        r.b[i] = add_halves(x[0].b[i]);
    }
    return r;
}

// the 16 bytes at p by a load the compiler does not count: it would wait vmcnt(0) for its own
// load — with it the LDS-DMA loads in flight, which it cannot see.  wait_vm<N>() + keep() instead.
__device__ __forceinline__ f32x4 load16_uncounted(const f32x4* p) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off nt" : "=&v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ void keep(f32x4& v) { asm volatile("" : "+v"(v)); }   // no use of v may move above this

__device__ __forceinline__ const NormArgs& norm_args(const NormArgs& na) { return na; }   // the one member of the kernel's pack

// NORM: the end of a workgroup's walk — the ticket, and for the last arriver the per-rank sums.
// ticket: 4 bytes of LDS that only wave 0 has used (`part`: it is done with it); tb: 512 bytes of LDS
// free once every wave is past its last tile (the tile buffers).
template <int P>
__device__ __forceinline__ void norm_finish(const NormArgs& na, const GroupSpan& span, uint32_t* ticket, uint2* tb, int lane,
                                            int w) {
    global_rw_u32* counter = (global_rw_u32*)na.ws;
    // thread t's entry of the finalizer's table, asked for ahead of the ticket (wave 0 holds all 64): its
    // round trip hides behind the drain instead of standing in the finalizer's serial path
    uint2 entry{};
    if (threadIdx.x < kGroupMax) entry = make_uint2(span.b[threadIdx.x].first, span.b[threadIdx.x].tpb);
    asm volatile("" : "+v"(entry.x), "+v"(entry.y));   // not to be sunk to its use behind the barriers
    if (w == 0) {
        wait_vm<0>();   // the storing wave's partials are written through
        if (lane == 0) {
            const uint32_t t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!kNormSc1Loads && t == span.G - 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            *ticket = t;
        }
        wait_vm<0>();   // the invalidate has happened before the barrier lets the readers go
    }
    __syncthreads();
    if (*ticket != span.G - 1) return;
    // every wave is past its last tile and no LDS-DMA is in flight: the tile buffers hold the
    // launch's (first tile, tiles per block) table for the lane-divergent walk below
    if (threadIdx.x < kGroupMax) tb[threadIdx.x] = entry;
    __syncthreads();
    constexpr int RW = P / 4;             // ranks of this wave: w + 4 r
    const uint32_t L = span.T / P;        // partials per rank: every bucket is P blocks of tpb tiles
    const float* partials = reinterpret_cast<const float*>(static_cast<const char*>(na.ws) + kNormCounterBytes) + na.tile_off;
    float a[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) a[r] = 0.0f;
    uint32_t k = 0, base = 0;             // this lane's cursor: bucket k holds partials [base, base + tpb) of a rank
    for (uint32_t m0 = 0; m0 < L; m0 += 64) {
        const uint32_t m = m0 + (uint32_t)lane;
        if (m < L) {
            uint2 e = tb[k];
            while (m - base >= e.y) {
                base += e.y;
                e = tb[++k];
            }
            const float* at = partials + e.x + (m - base);
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const float* p = at + (uint32_t)(w + 4 * r) * e.y;
                if constexpr (kNormSc1Loads)
                    a[r] = a[r] + __uint_as_float(__hip_atomic_load((global_rw_u32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                else
                    a[r] = a[r] + *p;
            }
        }
    }
    float out = 0.0f;
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        float t = a[r];
        t = add_halves(add_lanes32(t));
        if (lane == r) out = t;
    }
    if (lane < RW) {
        float* dst = na.norm_sq + (w + 4 * lane);
        if (na.launch > 0) out = *dst + out;
        *dst = out;
    }
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// k_tree_group_f32<P, ACC>: k_tree_group's one-row walk — persistent grid,
// workgroup g takes tiles g + j * G, a forward-only wave-uniform cursor over
// GroupSpan, two LDS tile buffers filled by LDS-DMA, the order table staged
// once, the next tile located before the wait — with the tree in fp32.
//
// Lane (q, c) = (lane / 32, lane % 32) of wave w widens its LPL = P / 8 leaves
// of column c (tree positions RPW w + LPL q ..) and adds them, one
// v_permlane32_swap level joins the two halves, and the four waves' partials
// meet in `part`: 32 bytes per column and wave, lane (q, c) writing 16-byte
// half q.  Wave 0 then joins: lane (q, c) adds half q of column c of the four
// partials — (p0 + p1) + (p2 + p3) —, multiplies by scale, ACC: adds the old
// 16 bytes, and stores; the 64 lanes' 16 bytes at (2 c + q) * 16 are the tile's
// contiguous 1 KiB of floats, ONE store instruction per tile.
//
// LDS: 2 x P x 512 (tiles) + 4096 (part) + P x 64 (order): 73,728 bytes at
// P = 64, two workgroups per CU in the 160 KiB.
//
// vmcnt, per wave, in issue order (L: a tile's OPS LDS-DMA loads, S: wave 0's
// result store, A: ACC's load of the old 16 bytes; waves 1-3 issue L only and
// wait vmcnt(0) for it, nothing else being in flight):
//   !ACC  L0 | L1 S0 | L2 S1 | ...      before tile j: L(j) S(j-1) outstanding,
//         vmcnt(1) leaves S(j-1) in flight (vmcnt(0) at j = 0) — k_tree_group's.
//   ACC   L0 A0 | L1 S0 A1 | L2 S1 A2 | ...   A(j) goes out right before the
//         wait for L(j), so its round trip overlaps that wait, the reduction
//         and the join.  Before tile j: L(j) S(j-1) A(j) outstanding — vmcnt(2)
//         (vmcnt(1) at j = 0, no store yet).  Before the add: behind A(j) are
//         L(j+1)'s OPS loads, or nothing after the last tile: vmcnt(OPS) / vmcnt(0).
// The !ACC instance holds no shard load at all (if constexpr).
// The shard tile of a workgroup is read (ACC) and written by wave 0 of that
// workgroup alone, and no other tile of the launch touches it (the lists are
// block-disjoint: engine.cpp shards_f32_check).
//
// NORM (k_tree_group_f32_norm; the other instances hold none of this: if
// constexpr): norm_sq[b] = the sum of the squares of every float v this launch
// stores into block b, in the fixed order allred.h states.
//   per tile   wave 0, which holds v: lane (q, c) has elements 4 (2 c + q) .. + 3
//              of the tile, so (x0^2 + x1^2) + (x2^2 + x3^2), then the level across
//              q (add_halves), then c bit 0 .. bit 4 by butterfly — the balanced
//              tree over the 256 squares in element order.  Lane 0 stores the
//              partial N to ws_partials[tile_off + global tile] by a relaxed
//              agent-scope atomic store: ONE write-through (sc1) vector store of 4
//              bytes, behind S in issue order.  vmcnt with N:
//   !ACC  L0 | L1 S0 N0 | L2 S1 N1 | ...   before tile j: L(j) S(j-1) N(j-1)
//         outstanding — vmcnt(2) leaves both stores in flight (vmcnt(0) at j = 0).
//   ACC   L0 A0 | L1 S0 N0 A1 | L2 S1 N1 A2 | ...   before tile j: L(j) S(j-1)
//         N(j-1) A(j) — vmcnt(3) (vmcnt(1) at j = 0).  Before the add nothing
//         changes: behind A(j) are L(j+1)'s OPS loads, or nothing.
//   at the end of the walk (the in-launch ticket reducer: a counter instead of a
//   flag, partials written through and drained, so no release fence): wave 0
//   waits vmcnt(0), lane 0 takes a ticket (relaxed agent-scope fetch_add on the
//   counter at the head of the workspace) — EVERY workgroup of the grid does, one
//   without tiles too.  The workgroup that draws G - 1 is the finalizer: that
//   lane's agent-scope acquire fence, vmcnt(0), __syncthreads(), then plain VECTOR
//   loads of the partials by all four waves.  Wave w takes ranks w, w + 4, ...:
//   rank b's partials in list order are, bucket by bucket, the tpb consecutive
//   floats of block b; lane l adds S[l], S[l + 64], ... from +0.0f, a 64-lane
//   butterfly is the tree over a_0 .. a_63, one lane adds what the previous
//   launch left in norm_sq[b] (launch > 0) and stores.  Thread 0 then puts the
//   counter back to 0 (agent-scope atomic store): the next launch, or replay,
//   finds it zero.  Nobody waits for another workgroup anywhere.
// ONE template for both: the pack Norm is empty (k_tree_group_f32<P, ACC>: the
// arguments and, instruction for instruction, the code of before) or NormArgs
// (k_tree_group_f32_norm<P, ACC>).  A bool on a shared __device__ body under
// two __global__ wrappers did not keep the old instances' code.
// ---------------------------------------------------------------------------
template <int P, bool ACC, class... Norm>
__global__ __launch_bounds__(kBlock) void k_tree_group_f32(const uint8_t* __restrict__ order, GroupSpan span,
                                                           GroupShardsF32 shards, float scale, Norm... norm) {
    constexpr bool NORM = sizeof...(Norm) == 1;
    static_assert(sizeof...(Norm) <= 1 && (std::is_same_v<Norm, NormArgs> && ...), "Norm: nothing, or NormArgs");
    constexpr int TV = 32, RPI = 2, RPW = P / 4, OPS = RPW / RPI, LPL = OPS;
    static_assert(OPS >= 1, "P >= 8");
    __shared__ __attribute__((aligned(16))) uint4 buf[2][P * TV];
    __shared__ __attribute__((aligned(16))) f32x4 part[4 * TV * 2];
    __shared__ __attribute__((aligned(16))) uint8_t ord_lds[P * ALLRED_MAX_NODES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane % TV, q = lane / TV;
    const uint32_t wbase = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&buf[0][0] + (uint32_t)(RPW * w * TV * 16));
    struct Tile {
        uint16_t* ranks;   // the bucket's row 0
        uint64_t stride;
        uint64_t v0;       // the tile's first 16-byte vector inside a rank row
        uint32_t block;
        f32x4* dst;        // the tile's 1 KiB of the shard
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        Tile t;
        t.ranks = span.b[gt.bucket].ranks;
        t.stride = span.b[gt.bucket].stride;
        t.v0 = (uint64_t)gt.local * TV;
        t.block = gt.block;
        t.dst = reinterpret_cast<f32x4*>(shards.s[gt.bucket].shard + (uint64_t)gt.block * shards.s[gt.bucket].stride) +
                (uint64_t)gt.rem * (2 * TV);
        return t;
    };
    auto issue = [&](const Tile& t, int b) {
#pragma unroll
        for (int k = 0; k < OPS; ++k) {
            const int r = RPW * w + RPI * k + q;
            const uint4* src = reinterpret_cast<const uint4*>(t.ranks + (uint64_t)r * t.stride) + t.v0 + c;
            lds_dma16(src, wbase + (uint32_t)(b * P * TV * 16 + RPI * k * TV * 16));
        }
    };
    const int mine = (int)group_span_mine(span, blockIdx.x);
    // the order rows of all P blocks, once, then the first tile's loads
    for (int i = threadIdx.x; i < P * ALLRED_MAX_NODES / 16; i += kBlock)
        reinterpret_cast<uint4*>(ord_lds)[i] = reinterpret_cast<const uint4*>(order)[i];
    __syncthreads();
    if (mine <= 0) {
        if constexpr (NORM) norm_finish<P>(norm_args(norm...), span, reinterpret_cast<uint32_t*>(&part[0]), reinterpret_cast<uint2*>(&buf[0][0]), lane, w);
        return;
    }
    Tile cur = locate(0), nxt = cur;
    issue(cur, 0);
    for (int j = 0; j < mine; ++j) {
        if (j + 1 < mine) nxt = locate(j + 1);
        f32x4 old{};
        if (w == 0) {
            constexpr int N = NORM ? 1 : 0;   // the partial's store, in flight behind S
            if constexpr (ACC) {
                old = load16_uncounted(cur.dst + (2 * c + q));
                if (j > 0) wait_vm<2 + N>(); else wait_vm<1>();
            } else {
                if (j > 0) wait_vm<1 + N>(); else wait_vm<0>();
            }
        } else {
            wait_vm<0>();
        }
        lds_barrier();
        if (j + 1 < mine) issue(nxt, (j + 1) & 1);
        const uint4* tile = buf[j & 1];
        const F8 pw = tree_wave_part_f32<TV, LPL>(tile, ord_lds + cur.block * ALLRED_MAX_NODES + RPW * w + LPL * q, c);
        part[(w * TV + c) * 2 + q] = q ? pw.b : pw.a;
        lds_barrier();
        if (w == 0) {
            const f32x4 s = (part[(0 * TV + c) * 2 + q] + part[(1 * TV + c) * 2 + q]) +
                            (part[(2 * TV + c) * 2 + q] + part[(3 * TV + c) * 2 + q]);
            f32x4 v = s * scale;
            if constexpr (ACC) {
                if (j + 1 < mine) wait_vm<OPS>(); else wait_vm<0>();
                keep(old);
                v = old + v;
            }
            __builtin_nontemporal_store(v, (global_f32x4*)(cur.dst + (2 * c + q)));
            if constexpr (NORM) {
                const NormArgs& na = norm_args(norm...);
                const f32x4 sq = v * v;
                float t = (sq[0] + sq[1]) + (sq[2] + sq[3]);
                t = add_lanes32(add_halves(t));
                if (lane == 0)
                    __hip_atomic_store((global_rw_u32*)(static_cast<char*>(na.ws) + kNormCounterBytes) + (na.tile_off + group_span_tile(span, blockIdx.x, (uint32_t)j)),
                                       __float_as_uint(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        cur = nxt;
    }
    if constexpr (NORM) norm_finish<P>(norm_args(norm...), span, reinterpret_cast<uint32_t*>(&part[0]), reinterpret_cast<uint2*>(&buf[0][0]), lane, w);
}

// the instances with the norm: k_tree_group_f32<P, ACC, NormArgs>, traced as k_tree_group_f32_norm<P, ACC>
template <int P, bool ACC>
constexpr auto k_tree_group_f32_norm = k_tree_group_f32<P, ACC, NormArgs>;

// ---------------------------------------------------------------------------
// k_ag_group_f32<P>: k_ag_group's walk and store loop from an fp32 shard.  A
// tile's source is wave-uniform: 1 KiB of floats in ONE block of the shard, at
// shard + b * stride + rem * 256.  Lane c loads its 32 bytes — the 8 floats of
// column c — as two 16-byte loads (both lane halves q load the same data),
// rounds them once to bf16 (pack_rne: IEEE RNE, Inf kept, NaN stays NaN, no
// flushing) into one uint4 and stores that to its rows r = RPW w + RPI k + q.
// Every row is written — there is no in-place case — and the shard only read.
// What keeps the compiler's waits exact is k_ag_group's: unconditional loads and
// stores, two tiles per trip with registers of their own, tile 0 peeled.  Issue
// order per wave: L0 L1 S0 L2 S1 L3 S2 ... with L two loads and S OPS stores:
// behind tile j's loads come tile j - 1's OPS stores and tile j + 1's two loads,
// so the wait before tile j's stores is vmcnt(OPS + 2) — and that is what the
// ISA has in the loop, twice, and nothing else (vmcnt(2) before the peeled tile
// 0, vmcnt(OPS) before an odd last tile; what it took: below and DESIGN.md §13).
// ---------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kBlock) void k_ag_group_f32(GroupSpan span, GroupShardsF32 shards) {
    constexpr int TV = 32, RPI = 2, RPW = P / 4, OPS = RPW / RPI;
    static_assert(OPS >= 1, "P >= 8");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane % TV, q = lane / TV;
    struct Tile {
        uint16_t* ranks;   // the bucket's row 0
        uint64_t stride;
        uint64_t v0;       // the tile's first 16-byte vector inside a rank row
        const f32x4* src;  // the source tile's first 16 bytes
    };
    uint32_t cursor = 0;   // wave-uniform: it depends on blockIdx and j only
    auto locate = [&](int j) {
        const GroupTile gt = group_span_at(span, group_span_tile(span, blockIdx.x, (uint32_t)j), cursor);
        const GroupBucket& e = span.b[gt.bucket];
        const GroupShardF32& sh = shards.s[gt.bucket];
        return Tile{e.ranks, e.stride, (uint64_t)gt.local * TV,
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
        // The conversions use the loaded floats, so the wait stands in front of THEM, not of the stores.
        // Without this barrier the scheduler lifts a conversion above the next tile's loads and the
        // wait goes with it: vmcnt(OPS), the next tile's loads issued only after this tile's landed.
        __builtin_amdgcn_sched_barrier(0);
        const uint4 v = make_uint4(pack_rne(x.a[0], x.a[1]), pack_rne(x.a[2], x.a[3]), pack_rne(x.b[0], x.b[1]),
                                   pack_rne(x.b[2], x.b[3]));
#pragma unroll
        for (int k = 0; k < OPS; ++k) {
            const uint32_t r = (uint32_t)(RPW * w + RPI * k + q);
            st_nt(reinterpret_cast<uint4*>(t.ranks + (uint64_t)r * t.stride) + t.v0 + c, v);
        }
    };
    // the "next" tile's loads are unconditional: a workgroup's last tile is loaded once more (an L2 hit)
    auto at = [&](int j) { return locate(j < last ? j : last); };
    Tile a = locate(0);
    Src xa = load(a);
    Tile b = at(1);
    Src xb = load(b);
    store(a, xa);
    // The odd tile behind the pairs is stored after the loop, not by a break out of its middle: the
    // structurised break joins the loop's latch, and the compiler, which then sees tile j + 2's
    // registers as possibly in flight at the loop's head, waits vmcnt(OPS + 1) before it reuses one
    // as a temporary — tile j + 1's first load drained ahead of tile j + 2's (seen in the ISA).
    int j = 1;
    for (; j + 1 < mine; j += 2) {
        a = at(j + 1);
        xa = load(a);
        store(b, xb);   // tile j
        b = at(j + 2);
        xb = load(b);
        store(a, xa);   // tile j + 1
    }
    if (j < mine) store(b, xb);   // the last tile of an even count: behind its loads only tile j - 1's stores, vmcnt(OPS)
}
// k_ag_group's resident cap (tune pipe_grid caps it lower): 8 four-wave workgroups per CU
constexpr uint64_t kAgGroupGrid = kMaxGrid;

}  // namespace

// A (checked: engine.cpp shards_f32_check) list of whole-tile buckets with fp32 shards through
// k_tree_group_f32 (ALLRED_OP_REDUCE_SCATTER) or k_ag_group_f32 (ALLRED_OP_ALL_GATHER), kGroupMax
// buckets per launch, enqueued when its last member is reached.  EVERY bucket takes this route:
// there is one kernel form for fp32 shards — a 64-rank bucket of >= 1024 tiles stays here too (no
// fp32 form of k_tree_lds_lag exists and nobody has measured where one would pay), and fused_form
// does not apply.  dry: nothing is launched and the number of launches is returned.
// norm_sq != nullptr (reduce-scatter only): the same launches as k_tree_group_f32_norm, launch k
// with the partials' region behind the tiles of launches 0 .. k - 1 of norm_ws.
int launch_shard_group_f32(const allred_shard_bucket_f32* buckets, int count, int total, const uint8_t* order, int op,
                           float scale, bool accumulate, bool dry, void* stream, float* norm_sq, void* norm_ws) {
    const bool gather = op == ALLRED_OP_ALL_GATHER;
    if (gather && norm_sq) return ALLRED_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    GroupShardsF32 shards{};
    auto add = [&](int i, int slot) {
        const allred_shard_bucket_f32& b = buckets[i];
        const uint64_t nv = b.elems_per_rank / 8, bv = nv / total, tiles = nv / 32;
        if (total < 8 || nv % 32 || bv % 32) return BatchAdd::error(ALLRED_ERR_UNSUPPORTED);   // the caller's check, kept next to its use
        shards.s[slot] = GroupShardF32{b.shard, b.shard_stride};
        return BatchAdd::member(GroupIn{b.ranks, b.rank_stride, tiles, bv / 32});
    };
    auto launch = [&](const GroupSpan& span, unsigned grid, int index, uint64_t tile_off) {
        const NormArgs na{norm_sq, norm_ws, (uint32_t)tile_off, (uint32_t)index};
        const bool found = for_ranks<8, 64>(total, [&](auto p) {
            if (norm_sq) {
                if (accumulate)
                    hipLaunchKernelGGL((k_tree_group_f32_norm<p(), true>), dim3(grid), dim3(kBlock), 0, st, order, span, shards, scale, na);
                else
                    hipLaunchKernelGGL((k_tree_group_f32_norm<p(), false>), dim3(grid), dim3(kBlock), 0, st, order, span, shards, scale, na);
                trace_launch(grid, kBlock, "k_tree_group_f32_norm<%d, %s>", total, tf(accumulate));
                return;
            }
            if (gather) hipLaunchKernelGGL((k_ag_group_f32<p()>), dim3(grid), dim3(kBlock), 0, st, span, shards);
            else if (accumulate)
                hipLaunchKernelGGL((k_tree_group_f32<p(), true>), dim3(grid), dim3(kBlock), 0, st, order, span, shards, scale);
            else hipLaunchKernelGGL((k_tree_group_f32<p(), false>), dim3(grid), dim3(kBlock), 0, st, order, span, shards, scale);
            if (gather) trace_launch(grid, kBlock, "k_ag_group_f32<%d>", total);
            else trace_launch(grid, kBlock, "k_tree_group_f32<%d, %s>", total, tf(accumulate));
        });
        return found ? last_error() : ALLRED_ERR_UNSUPPORTED;
    };
    // the tree pass on 2 workgroups per CU like every tree pass (LDS-bound); the copy, which
    // holds no LDS, on up to kAgGroupGrid workgroups like k_ag_group
    return group_batch<kGroupMax>(count, dry, shards, add,
                                  [&](uint64_t tiles) { return persistent_grid(tiles, gather ? kAgGroupGrid : 512); }, launch);
}

}  // namespace tsa
