// TEST INFRASTRUCTURE ONLY — never linked into liballred.so.
//
// The two kernels of the replay soak (tests/soak.py) that are not the library's:
//
//   k_soak_load        the memory load the soaked kernels run under: a bounded streaming pass over a
//                      scratch buffer.  Workgroup g, iteration k reads and rewrites the 16-byte vector
//                      (start + (k * G + g) * 256 + thread) & mask of the buffer.  `mask` + 1 is the
//                      buffer's size in vectors (a power of two), so every index is inside it whatever
//                      the grid, the start and the iteration count.  No flags, no waits.
//
//   k_ticket_sum<MODE> THE CONTROL: a self-contained copy of the SHAPE of the ticket reducer at the
//                      end of k_tree_group_f32_norm (shard_f32_kernels.hip, norm_finish), with a payload
//                      a compare can decide.  G workgroups of 256 threads.  Workgroup g:
//                        1. thread 0 stores in[g] to partials[g];
//                        2. every thread pre-reads the partial lines by plain loads, so that this
//                           CU's L1 holds them BEFORE most of them are written (the L1-warm consumer
//                           that a cold test never is);
//                        3. thread 0 takes a ticket (relaxed agent-scope fetch_add);
//                        4. the workgroup that draws G - 1 reads all G partials by plain loads, counts
//                           those that differ from `in`, writes the count to out[0] and the counter
//                           back to 0.
//                      MODE 0, the product's form: the store of step 1 is a relaxed agent-scope atomic
//                        store (one write-through vector store), drained by vmcnt(0) before the ticket;
//                        the last arriver's lane runs an agent-scope acquire fence and vmcnt(0) before
//                        the barrier that lets the readers go.  out[0] must be 0, always.
//                      MODE 1, the broken form, kept so that the soak can be shown to see it: a plain
//                        store, no release, no acquire.  out[0] is the number of stale partials.
//                      Nobody waits for anybody: every workgroup runs straight to its end whatever the
//                      others do, so no mode can hang.  The kernel writes partials[0 .. G), counter[0]
//                      and out[0] only; every store is a vector store or a vector atomic.
#include <hip/hip_runtime.h>

#include <cstdint>

typedef __attribute__((address_space(1))) uint32_t global_u32;

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_soak_load(uint4* __restrict__ buf, uint32_t mask, uint32_t start, uint32_t iters) {
    const uint32_t lane = (uint32_t)blockIdx.x * kThreads + threadIdx.x;
    const uint32_t step = (uint32_t)gridDim.x * kThreads;
#pragma unroll 4
    for (uint32_t k = 0; k < iters; ++k) {
        uint4* p = buf + ((start + k * step + lane) & mask);
        uint4 v = *p;
        v.x += 1u;
        *p = v;
    }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_ticket_sum(const uint32_t* in, uint32_t* partials, uint32_t* counter, uint32_t* out) {
    __shared__ uint32_t ticket, differing;
    const uint32_t G = gridDim.x, g = blockIdx.x;
    if (threadIdx.x == 0) {
        differing = 0;
        if constexpr (MODE == 0)
            __hip_atomic_store((global_u32*)(partials + g), in[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            partials[g] = in[g];
    }
    asm volatile("" ::: "memory");
    // the pre-read: plain loads of every partial line into this CU's L1; the values are kept alive, not used
    uint32_t seen = 0;
    for (uint32_t i = threadIdx.x; i < G; i += kThreads) seen += partials[i];
    asm volatile("" : "+v"(seen)::"memory");
    if (threadIdx.x == 0) {
        if constexpr (MODE == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the partial is written through
        const uint32_t t = __hip_atomic_fetch_add((global_u32*)counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (MODE == 0) {
            if (t == G - 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the invalidate has happened before the barrier
        }
        ticket = t;
    }
    __syncthreads();
    if (ticket != G - 1) return;
    asm volatile("" ::: "memory");
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < G; i += kThreads) bad += partials[i] != in[i];
    if (bad) atomicAdd(&differing, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = differing;
        __hip_atomic_store((global_u32*)counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// 0, -1 for arguments the kernel cannot take, or the HIP error of the launch.
// buf: `vectors` 16-byte vectors, a power of two.
extern "C" int soak_load(void* buf, uint64_t vectors, uint32_t start, uint32_t iters, uint32_t grid, void* stream) {
    if (!buf || vectors == 0 || (vectors & (vectors - 1)) || vectors > (1ull << 32) || grid == 0 || grid > 65536) return -1;
    hipLaunchKernelGGL(k_soak_load, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, (uint4*)buf, (uint32_t)(vectors - 1), start, iters);
    return (int)hipGetLastError();
}

// in, partials: G words each; counter: one word, zero before the first launch; out: one word.
extern "C" int ticket_sum(int mode, const uint32_t* in, uint32_t* partials, uint32_t* counter, uint32_t* out, uint32_t G,
                          void* stream) {
    if (!in || !partials || !counter || !out || G == 0 || G > 65536 || (mode != 0 && mode != 1)) return -1;
    if (mode == 0)
        hipLaunchKernelGGL(k_ticket_sum<0>, dim3(G), dim3(kThreads), 0, (hipStream_t)stream, in, partials, counter, out);
    else
        hipLaunchKernelGGL(k_ticket_sum<1>, dim3(G), dim3(kThreads), 0, (hipStream_t)stream, in, partials, counter, out);
    return (int)hipGetLastError();
}
