// validate_time.cpp — k_validate (allred_validate_device) at config 2: 64 rows x 327,680 bf16 on
// the skewed stride, a correct bucket (expected = RNE((a + b) * 32) in every row).
//   kernel     hipEvents around `reps` back-to-back launches (tsa::launch_validate), after a warm-up;
//              algorithmic bytes = rows * n * 2 + 2 * n * 2 = 43,253,760
//   call       allred_validate_device as a caller sees it: two memsets, the launch, the copy of the
//              records, the synchronise (host clock)
//   tree       the yardstick on the same box: the read-only tree over the same rows
//              (allred_tree_reduce -> k_tree_lds_pipe<64, false>), hipEvents, same reps
//   host_loop  what ALLRED_CHECK_ALL=1 does after a DMA-mode run: the rows to pinned host memory
//              (one pass out of the skewed layout + one D2H copy) and 64 host validations (host clock)
// Prints one JSON line.  Host-only C++ against liballred.so's internal launchers:
//   hipcc -O2 -std=c++17 -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include \
//         -I../../tenstorrentallreduce_amd/csrc \
//         validate_time.cpp -o validate_time -L../../tenstorrentallreduce_amd/lib -lallred \
//         -Wl,-rpath,'$ORIGIN/../../tenstorrentallreduce_amd/lib' -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "internal.hpp"

#define CK(x)                                                                      \
    do {                                                                           \
        if ((x) != hipSuccess) { std::fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return 1; } \
    } while (0)
#define OK(x)                                                                      \
    do {                                                                           \
        const int s_ = (x);                                                        \
        if (s_ != ALLRED_OK) { std::fprintf(stderr, "status %d at %s:%d\n", s_, __FILE__, __LINE__); return 1; } \
    } while (0)

using clk = std::chrono::steady_clock;
static double us_since(clk::time_point t0) { return std::chrono::duration<double, std::micro>(clk::now() - t0).count(); }

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::max(50, std::atoi(argv[1])) : 100;
    const int N = 64, rounds = 3;
    const size_t n = 327680, bytes = n * 2, stride = (size_t)allred_preferred_rank_stride(n);
    const float mult = 32.0f;
    setenv("ALLRED_BF16_ROUND", "rne", 1);   // the host validator's conversion
    std::vector<uint32_t> s0(n / 2), s1(n / 2);
    allred_random_bf16_vector(bytes, 100, 13, 1, s0.data());
    allred_random_bf16_vector(bytes, 100, 14, 1, s1.data());
    const uint16_t* a = reinterpret_cast<const uint16_t*>(s0.data());
    const uint16_t* b = reinterpret_cast<const uint16_t*>(s1.data());
    std::vector<uint16_t> rows((size_t)N * stride, 0xFFFF);
    for (size_t i = 0; i < n; ++i) {
        const uint16_t e = tsa::bf16_from_float_rne((tsa::bf16_to_float(a[i]) + tsa::bf16_to_float(b[i])) * mult);
        for (int r = 0; r < N; ++r) rows[(size_t)r * stride + i] = e;
    }
    uint16_t *d_rows = nullptr, *d_src = nullptr, *d_stage = nullptr, *d_out = nullptr, *h_pin = nullptr;
    tsa::ValidateCounters* d_ctr = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    CK(hipMalloc((void**)&d_rows, rows.size() * 2));
    CK(hipMalloc((void**)&d_src, 2 * bytes));
    CK(hipMalloc((void**)&d_stage, (size_t)N * bytes));
    CK(hipMalloc((void**)&d_out, bytes));
    CK(hipMalloc((void**)&d_ctr, sizeof(*d_ctr)));
    CK(hipHostMalloc((void**)&h_pin, (size_t)N * bytes, hipHostMallocDefault));
    CK(hipMemcpy(d_rows, rows.data(), rows.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_src, a, bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_src + n, b, bytes, hipMemcpyHostToDevice));
    CK(hipMemset(d_ctr, 0, sizeof(*d_ctr)));

    // correctness first: every row clean, on the device and on the host
    std::vector<allred_rank_check> rec(N);
    OK(allred_validate_device(d_rows, stride, n, N, d_src, d_src + n, mult, 0.0f, 1, rec.data(), s));
    uint64_t bad = 0;
    for (const auto& x : rec) bad += x.bad;

    double kern[rounds], tree[rounds], call[rounds], host[rounds];
    long host_bad = 0;
    for (int i = 0; i < 10; ++i) {   // warm-up of both kernels
        OK(tsa::launch_validate(d_rows, stride, n, N, d_src, d_src + n, mult, 0.0f, true, d_ctr, s));
        OK(allred_tree_reduce(d_rows, stride, n, ALLRED_SWING, 8, N, d_out, s));
    }
    CK(hipStreamSynchronize(s));
    for (int k = 0; k < rounds; ++k) {
        float ms = 0;
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i)
            OK(tsa::launch_validate(d_rows, stride, n, N, d_src, d_src + n, mult, 0.0f, true, d_ctr, s));
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        CK(hipEventElapsedTime(&ms, e0, e1));
        kern[k] = ms * 1e3 / reps;
        CK(hipEventRecord(e0, s));
        for (int i = 0; i < reps; ++i) OK(allred_tree_reduce(d_rows, stride, n, ALLRED_SWING, 8, N, d_out, s));
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        CK(hipEventElapsedTime(&ms, e0, e1));
        tree[k] = ms * 1e3 / reps;
        auto t0 = clk::now();
        for (int i = 0; i < 20; ++i)
            OK(allred_validate_device(d_rows, stride, n, N, d_src, d_src + n, mult, 0.0f, 1, rec.data(), s));
        call[k] = us_since(t0) / 20;
        t0 = clk::now();
        OK(tsa::launch_copy_ranks(d_rows, stride, d_stage, n, N, n, s));
        CK(hipMemcpyAsync(h_pin, d_stage, (size_t)N * bytes, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        host_bad = 0;
        for (int r = 0; r < N; ++r)
            host_bad += allred_validate_result_vector(reinterpret_cast<const uint32_t*>(h_pin + (size_t)r * n), s0.data(),
                                                      s1.data(), n / 2, 0.0f, 64, 0, nullptr);
        host[k] = us_since(t0);
    }
    const double algo_bytes = (double)N * bytes + 2.0 * bytes;
    std::sort(kern, kern + rounds);
    std::sort(tree, tree + rounds);
    std::sort(call, call + rounds);
    std::sort(host, host + rounds);
    std::printf("{\"rows\": %d, \"elems\": %zu, \"stride\": %zu, \"reps\": %d, \"rounds\": %d, \"device_bad\": %llu, "
                "\"host_bad\": %ld, \"algo_bytes\": %.0f, \"k_validate_us\": [%.2f, %.2f, %.2f], "
                "\"k_validate_TBps_median\": %.3f, \"k_validate_of_8TBps_median\": %.3f, "
                "\"tree_reduce_us\": [%.2f, %.2f, %.2f], \"validate_device_call_us\": [%.1f, %.1f, %.1f], "
                "\"host_loop_us\": [%.0f, %.0f, %.0f]}\n",
                N, n, stride, reps, rounds, (unsigned long long)bad, host_bad, algo_bytes, kern[0], kern[1], kern[2],
                algo_bytes / (kern[1] * 1e-6) / 1e12, algo_bytes / (kern[1] * 1e-6) / 8e12, tree[0], tree[1], tree[2],
                call[0], call[1], call[2], host[0], host[1], host[2]);
    return bad == 0 && host_bad == 0 ? 0 : 1;
}
