// rs_ag_kernels.hip — the two halves of the BO allreduce as passes of their own
// (allred_plan_reduce_scatter / allred_plan_all_gather, fused plans), P ranks
// resident in one GPU's HBM.
//
// Reduce-scatter (the RS loop of allred_BO_2D/kernels/dataflow_kernel.cpp:152-213
// + compute_kernel.cpp:35-67): block b of the result is tree b of the schedule
// (leaf order order[b], level k adds adjacent groups of 2^k leaves, every add
// rounded to bf16) — the trees, leaf orders and add order of k_tree / k_tree_lds
// (kernels.hip), so the bits are those of the fused BO pass.  The pass reads
// the P rank rows of every tile and writes ONE row's worth: block b to rank b's
// row (in place) or to out + b * out_stride.  (P + 1) n bytes instead of 2 P n.
// All-gather (the AG loop, dataflow_kernel.cpp:219-267): block b of rank b (or
// of in + b * in_stride) copied to block b of every rank, a pure 16-bit copy.
//
// In place, a tile of block b is read (all P rows) and written (row b) by one
// workgroup — in the register form by one wave — and every load of the tile
// has landed before the store goes out (the store's data depends on them
// through the shuffles, or a barrier stands between); no other workgroup
// touches that tile.
#include "device.hpp"

namespace tsa {
namespace {

// where the result vector v (16-byte index in a rank row) of block b goes
__device__ __forceinline__ uint4* rs_dst(uint16_t* ranks, uint64_t stride, uint16_t* out, uint64_t out_stride,
                                         uint64_t b, uint64_t v, uint64_t block_vec) {
    return out ? reinterpret_cast<uint4*>(out + b * out_stride) + (v - b * block_vec)
               : reinterpret_cast<uint4*>(ranks + b * stride) + v;
}

// ---------------------------------------------------------------------------
// Register form (P < 8, and buckets that are not whole 256-element tiles):
// k_tree's lane layout — lane = g * CH + c, the P / LEAVES lanes of chunk
// column c each reduce LEAVES leaves, xor-shuffles finish the tree — with the
// block, its order row and its destination PER LANE: with blocks shorter than
// a wave's CH chunks, the lanes of one wave fall into different blocks.  (All
// lanes of a column share v, hence b, so the shuffles combine one block's
// leaves.)  Lane g == 0 stores the column's result.
// ---------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kBlock) void k_rs_reg(uint16_t* __restrict__ ranks, uint64_t stride, uint64_t n_vec,
                                                   const uint8_t* __restrict__ order, uint64_t block_vec,
                                                   uint16_t* __restrict__ out, uint64_t out_stride) {
    constexpr int LEAVES = P >= 8 ? 8 : P;  // leaves per lane
    constexpr int LANES = P / LEAVES;        // lanes per chunk
    constexpr int CH = 64 / LANES;           // chunks per wave
    const int lane = threadIdx.x & 63;
    const int g = lane / CH;
    const int c = lane % CH;
    const uint4* rows[LEAVES];
    uint64_t cur = ~0ull;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
    for (uint64_t base = wave * CH; base < n_vec; base += waves * CH) {
        const uint64_t v = base + c;
        const bool ok = v < n_vec;
        const uint64_t b = ok ? v / block_vec : 0;
        if (b != cur) {
            cur = b;
#pragma unroll
            for (int i = 0; i < LEAVES; ++i)
                rows[i] = reinterpret_cast<const uint4*>(
                    ranks + (uint64_t)order[b * ALLRED_MAX_NODES + g * LEAVES + i] * stride);
        }
        uint4 x[LEAVES];
#pragma unroll
        for (int i = 0; i < LEAVES; ++i) x[i] = ok ? ld_nt(rows[i] + v) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int w = 1; w < LEAVES; w *= 2)
#pragma unroll
            for (int i = 0; i < LEAVES; i += 2 * w) x[i] = add8(x[i], x[i + w]);
        uint4 acc = x[0];
#pragma unroll
        for (int m = CH; m < 64; m *= 2) acc = add8(acc, shfl_xor4(acc, m));
        if (ok && g == 0) st_nt(rs_dst(ranks, stride, out, out_stride, b, v, block_vec), acc);
    }
}

// ---------------------------------------------------------------------------
// One tile per workgroup, staged in LDS (P >= 8, whole tiles): k_tree_lds's
// staging and tree — wave w stages ranks [P/4 w, P/4 (w+1)) by LDS-DMA and
// reduces tree positions [P/4 w, P/4 (w+1)) of every column, the four wave
// partials meet in LDS rows 0-3 — and one 512-byte store of the tile to its
// block's owner (or out) from the first 32 lanes.
// ---------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kBlock) void k_rs_lds(uint16_t* __restrict__ ranks, uint64_t stride,
                                                   const uint8_t* __restrict__ order, uint64_t block_vec,
                                                   uint16_t* __restrict__ out, uint64_t out_stride) {
    constexpr int TV = 32;          // 16-byte vectors per rank row of a tile
    constexpr int RPW = P / 4;      // ranks staged (and tree leaves reduced) per wave
    constexpr int LPL = RPW / 2;    // leaves per lane
    __shared__ __attribute__((aligned(16))) uint4 tile[P * TV];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const uint64_t v0 = (uint64_t)blockIdx.x * TV, b = v0 / block_vec;
#pragma unroll
    for (int k = 0; k < RPW / 2; ++k) {
        const int r = RPW * w + 2 * k + h;
        const uint4* src = reinterpret_cast<const uint4*>(ranks + (uint64_t)r * stride) + v0 + c;
        __builtin_amdgcn_global_load_lds((global_u32*)src, (lds_u32*)&tile[(RPW * w + 2 * k) * TV], 16, 0, 2);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint8_t* ord = order + b * ALLRED_MAX_NODES + RPW * w + LPL * h;
    uint4 x[LPL];
#pragma unroll
    for (int i = 0; i < LPL; ++i) x[i] = tile[(int)ord[i] * TV + c];
#pragma unroll
    for (int s = 1; s < LPL; s *= 2)
#pragma unroll
        for (int i = 0; i < LPL; i += 2 * s) x[i] = add8(x[i], x[i + s]);
    const uint4 part = add8(x[0], shfl_xor4(x[0], 32));
    __syncthreads();
    if (h == 0) tile[w * TV + c] = part;
    __syncthreads();
    if (w == 0 && h == 0) {
        const uint4 res = add8(add8(tile[0 * TV + c], tile[1 * TV + c]), add8(tile[2 * TV + c], tile[3 * TV + c]));
        st_nt(rs_dst(ranks, stride, out, out_stride, b, v0 + c, block_vec), res);
    }
}

// ---------------------------------------------------------------------------
// Persistent form (64 ranks from 1024 tiles): k_tree_lds_pipe<P, false>'s
// schedule — two LDS tile buffers, tile j+1's LDS-DMA loads issued before tile
// j is reduced, tiles of a workgroup blockIdx.x + j * G — with the order row of
// the tile's block and the result tile stored to the block's owner (or out).
// Exact vmcnt: wave 0 issues the one result store per tile and keeps tile
// j-1's in flight across the wait for tile j's loads (vmcnt(1): the store went
// out after them); the other waves have nothing but tile j's loads in flight.
// ---------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kBlock) void k_rs_pipe(uint16_t* __restrict__ ranks, uint64_t stride,
                                                    const uint8_t* __restrict__ order, uint64_t block_vec,
                                                    uint64_t ntiles, uint16_t* __restrict__ out, uint64_t out_stride) {
    constexpr int TV = 32, RPI = 2, RPW = P / 4, OPS = RPW / RPI, LPL = OPS;
    static_assert(OPS >= 1, "P >= 8");
    __shared__ __attribute__((aligned(16))) uint4 buf[2][P * TV];
    __shared__ __attribute__((aligned(16))) uint4 part[4 * TV];
    __shared__ __attribute__((aligned(16))) uint8_t ord_lds[P * ALLRED_MAX_NODES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane % TV, q = lane / TV;
    const uint32_t wbase = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&buf[0][0] + (uint32_t)(RPW * w * TV * 16));
    auto issue = [&](uint64_t t, int b) {
#pragma unroll
        for (int k = 0; k < OPS; ++k) {
            const int r = RPW * w + RPI * k + q;
            const uint4* src = reinterpret_cast<const uint4*>(ranks + (uint64_t)r * stride) + t * TV + c;
            lds_dma16(src, wbase + (uint32_t)(b * P * TV * 16 + RPI * k * TV * 16));
        }
    };
    const uint64_t G = gridDim.x;
    const int mine = blockIdx.x < ntiles ? (int)((ntiles - 1 - blockIdx.x) / G + 1) : 0;
    // the order rows of all P blocks, once, then the first tile's loads
    for (int i = threadIdx.x; i < P * ALLRED_MAX_NODES / 16; i += kBlock)
        reinterpret_cast<uint4*>(ord_lds)[i] = reinterpret_cast<const uint4*>(order)[i];
    __syncthreads();
    if (mine > 0) issue(blockIdx.x, 0);
    for (int j = 0; j < mine; ++j) {
        if (j > 0 && w == 0) wait_vm<1>();   // tile j-1's result store may stay in flight
        else wait_vm<0>();
        lds_barrier();   // every wave's rows of tile j are in LDS; everyone is done with tile j-1
        if (j + 1 < mine) issue(blockIdx.x + (uint64_t)(j + 1) * G, (j + 1) & 1);
        const uint4* tile = buf[j & 1];
        const uint64_t v0 = (blockIdx.x + (uint64_t)j * G) * TV, b = v0 / block_vec;
        const uint8_t* ord = ord_lds + b * ALLRED_MAX_NODES + RPW * w + LPL * q;
        uint4 x[LPL];
#pragma unroll
        for (int i = 0; i < LPL; ++i) x[i] = tile[(int)ord[i] * TV + c];
#pragma unroll
        for (int s = 1; s < LPL; s *= 2)
#pragma unroll
            for (int i = 0; i < LPL; i += 2 * s) x[i] = add8(x[i], x[i + s]);
        const uint4 pw = add8(x[0], shfl_xor4(x[0], 32));   // tree level across the two lane halves
        if (q == 0) part[w * TV + c] = pw;
        lds_barrier();
        if (w == 0 && q == 0) {
            const uint4 res = add8(add8(part[0 * TV + c], part[1 * TV + c]), add8(part[2 * TV + c], part[3 * TV + c]));
            st_nt(rs_dst(ranks, stride, out, out_stride, b, v0 + c, block_vec), res);
        }
    }
}

// ---------------------------------------------------------------------------
// All-gather: k_broadcast's data movement with the source row chosen per
// block, on a persistent grid.  A wave's item = (64 consecutive 16-byte
// vectors — two 512-byte tiles —, a group of up to 8 ranks): one load per lane
// from the vector's block owner (or `in`), then its 8 row stores; the next
// item's load goes out before the stores, so a wave never waits for a load
// with an empty store queue.  Items are group-major, so the waves of a
// workgroup write adjacent kilobytes of the same 8 rows.  The source block and
// row are per lane: a 64-vector run may cross blocks.  In place the owner's
// own row is not rewritten; every other row of a vector has exactly one writer
// and the source vector none, so there is nothing to order.
// ---------------------------------------------------------------------------
constexpr int kAgRows = 8;

__global__ __launch_bounds__(kBlock) void k_ag(uint16_t* ranks, uint64_t stride, int total, uint64_t n_vec,
                                               uint64_t block_vec, const uint16_t* in, uint64_t in_stride,
                                               uint64_t chunks, uint64_t items) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kBlock / 64);
    uint64_t i = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= items) return;
    auto load = [&](uint64_t item, uint64_t& v, uint64_t& b) {
        v = (item % chunks) * 64 + lane;
        b = v < n_vec ? v / block_vec : 0;
        if (v >= n_vec) return make_uint4(0, 0, 0, 0);
        return in ? reinterpret_cast<const uint4*>(in + b * in_stride)[v - b * block_vec]
                  : reinterpret_cast<const uint4*>(ranks + b * stride)[v];
    };
    uint64_t v, b, vn = 0, bn = 0;
    uint4 x = load(i, v, b), xn = make_uint4(0, 0, 0, 0);
    for (;;) {
        const uint64_t next = i + waves;
        const bool more = next < items;
        if (more) xn = load(next, vn, bn);
        const int r0 = (int)(i / chunks) * kAgRows;
        if (v < n_vec) {
#pragma unroll
            for (int k = 0; k < kAgRows; ++k) {
                const int r = r0 + k;
                if (r < total && (in || (uint64_t)r != b)) st_nt(reinterpret_cast<uint4*>(ranks + (uint64_t)r * stride) + v, x);
            }
        }
        if (!more) break;
        i = next, v = vn, b = bn, x = xn;
    }
}

int last_error() { return hip_status((int)hipGetLastError()); }

unsigned persistent_grid(uint64_t groups, uint64_t dflt) {
    const int64_t g = tune(Tune::pipe_grid);
    const uint64_t cap = g > 0 ? (uint64_t)g : dflt;
    return (unsigned)(groups < cap ? groups : cap);
}

}  // namespace

// The three shape classes of launch_tree_fused / tree_dispatch (kernels.hip), tune fused_form
// as there (0 auto, 1 register form, 2 one tile per workgroup, 3 persistent): 64 ranks from
// 1024 whole tiles -> k_rs_pipe; 8+ ranks in whole tiles -> k_rs_lds; everything else -> k_rs_reg.
int launch_reduce_scatter(uint16_t* ranks, uint64_t stride, size_t n, int total, const uint8_t* order, uint16_t* out,
                          uint64_t out_stride, void* stream) {
    if (total < 1 || n == 0 || n % (8 * (size_t)total) || stride % 8 || !aligned16(ranks) ||
        (out && (out_stride % 8 || !aligned16(out))))
        return ALLRED_ERR_ARG;
    const uint64_t nv = n / 8, bv = nv / total, tiles = nv / 32;
    const int64_t form = tune(Tune::fused_form);
    hipStream_t st = (hipStream_t)stream;
    const bool whole_tiles = total >= 8 && nv % 32 == 0 && bv % 32 == 0;
    if (whole_tiles && form != 1 && form != 2 && ((total == 64 && tiles >= 1024) || form == 3)) {
        const dim3 grid(persistent_grid(tiles, 512)), blk(kBlock);
        switch (total) {
            case 8: hipLaunchKernelGGL((k_rs_pipe<8>), grid, blk, 0, st, ranks, stride, order, bv, tiles, out, out_stride); break;
            case 16: hipLaunchKernelGGL((k_rs_pipe<16>), grid, blk, 0, st, ranks, stride, order, bv, tiles, out, out_stride); break;
            case 32: hipLaunchKernelGGL((k_rs_pipe<32>), grid, blk, 0, st, ranks, stride, order, bv, tiles, out, out_stride); break;
            case 64: hipLaunchKernelGGL((k_rs_pipe<64>), grid, blk, 0, st, ranks, stride, order, bv, tiles, out, out_stride); break;
            default: return ALLRED_ERR_UNSUPPORTED;
        }
        return last_error();
    }
    if (whole_tiles && form != 1) {
        const dim3 grid((unsigned)tiles), blk(kBlock);
        switch (total) {
            case 8: hipLaunchKernelGGL((k_rs_lds<8>), grid, blk, 0, st, ranks, stride, order, bv, out, out_stride); break;
            case 16: hipLaunchKernelGGL((k_rs_lds<16>), grid, blk, 0, st, ranks, stride, order, bv, out, out_stride); break;
            case 32: hipLaunchKernelGGL((k_rs_lds<32>), grid, blk, 0, st, ranks, stride, order, bv, out, out_stride); break;
            case 64: hipLaunchKernelGGL((k_rs_lds<64>), grid, blk, 0, st, ranks, stride, order, bv, out, out_stride); break;
            default: return ALLRED_ERR_UNSUPPORTED;
        }
        return last_error();
    }
    const int lanes = total >= 8 ? total / 8 : 1;
    const uint64_t chunk_groups = (nv + (64 / lanes) - 1) / (64 / lanes);  // one per wave
    uint64_t blocks = (chunk_groups + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 grid((unsigned)blocks), blk(kBlock);
    switch (total) {
        case 1: hipLaunchKernelGGL((k_rs_reg<1>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        case 2: hipLaunchKernelGGL((k_rs_reg<2>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        case 4: hipLaunchKernelGGL((k_rs_reg<4>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        case 8: hipLaunchKernelGGL((k_rs_reg<8>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        case 16: hipLaunchKernelGGL((k_rs_reg<16>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        case 32: hipLaunchKernelGGL((k_rs_reg<32>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        case 64: hipLaunchKernelGGL((k_rs_reg<64>), grid, blk, 0, st, ranks, stride, nv, order, bv, out, out_stride); break;
        default: return ALLRED_ERR_UNSUPPORTED;
    }
    return last_error();
}

// one kernel for every shape: its items are 64-vector runs whatever the block size
int launch_all_gather(uint16_t* ranks, uint64_t stride, size_t n, int total, const uint16_t* in, uint64_t in_stride,
                      void* stream) {
    if (total < 1 || total > ALLRED_MAX_NODES || n == 0 || n % (8 * (size_t)total) || stride % 8 || !aligned16(ranks) ||
        (in && (in_stride % 8 || !aligned16(in))))
        return ALLRED_ERR_ARG;
    const uint64_t nv = n / 8, bv = nv / total, chunks = (nv + 63) / 64;
    const uint64_t items = chunks * (uint64_t)((total + kAgRows - 1) / kAgRows);
    // a resident grid (at most 8 four-wave workgroups per CU; tune pipe_grid caps it lower) sized so
    // that every wave gets the same number of items: a fixed 512 workgroups left config 2's 5120
    // items at 2 or 3 per wave, 7.96 us against k_broadcast's 7.58 in the same run
    const uint64_t groups = (items + 3) / 4, cap = persistent_grid(kMaxGrid, kMaxGrid);
    const uint64_t per = (groups + cap - 1) / cap;
    const dim3 grid((unsigned)((groups + per - 1) / per));
    hipLaunchKernelGGL(k_ag, grid, dim3(kBlock), 0, (hipStream_t)stream, ranks, stride, total, nv, bv, in, in_stride,
                       chunks, items);
    return last_error();
}

}  // namespace tsa
