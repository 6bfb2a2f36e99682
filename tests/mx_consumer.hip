// TEST INFRASTRUCTURE ONLY — never linked into liballred.so.
//
// A consumer for the rows allred_plan_all_gather_shards_mxfp8 writes: it feeds e4m3 bytes and their
// LINEAR E8M0 scale rows, exactly as they lie in memory, to the block-scaled MFMA of gfx950,
// v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 on both sides, and returns the fp32 products.
// tests/test_gpu_mx_consumer.py first holds this file to plain integer arithmetic (its controls) and
// then uses it to ask the hardware what a byte pair means.
//
// out[m][n] = sum over k of A[m][k] * 2^(sa[m][k / 32] - 127) * B[n][k] * 2^(sb[n][k / 32] - 127)
//
// THE LANE MAP (wave64, one wave per 16 rows of A; established on the MI355X by the controls of
// tests/test_gpu_mx_consumer.py, which fail under any other):
//   lane l, with g = l >> 4, holds of A row l & 15 the 16 consecutive bytes k0 + 16 g .. + 15 in dwords 0 .. 3
//   and the 16 bytes k0 + 64 + 16 g .. + 15 in dwords 4 .. 7 — two halves of two DIFFERENT MX blocks —, and
//   alike of B column l & 15;
//   with opsel 0, byte 0 of lane l's scale register is the scale of the row's WHOLE MX block g of this k-step,
//   bytes k0 + 32 g .. + 31 (held by other lanes of the row): the byte at k0 / 32 + g of the linear scale row;
//   D register i of lane l is out[4 (l >> 4) + i][l & 15].
// (The first guess — a lane's 32 bytes are one MX block, k0 + 32 g .. + 31 — gives the right product under
// equal scales and a wrong one as soon as two groups of a row differ in scale.)
// No byte is repacked and no scale swizzled: two 16-byte loads and one byte load per lane and operand, from
// the rows as they lie.  Every load is a per-lane global load.
#include <hip/hip_runtime.h>

#include <cstdint>

typedef int   i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static __device__ inline i32x8 load_halves(const uint8_t* p) {   // p is 16-byte aligned
    const int4 lo = *reinterpret_cast<const int4*>(p);
    const int4 hi = *reinterpret_cast<const int4*>(p + 64);
    i32x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return v;
}

__global__ __launch_bounds__(64) void k_mx_consume(const uint8_t* __restrict__ a, uint64_t a_row_stride,
                                                   const uint8_t* __restrict__ a_scales, uint64_t a_scale_stride, uint64_t k,
                                                   const uint8_t* __restrict__ b, const uint8_t* __restrict__ b_scales,
                                                   float* __restrict__ out) {
    const unsigned l = threadIdx.x, rc = l & 15, g = l >> 4;
    const uint64_t row = 16ull * blockIdx.x + rc;
    const uint8_t* ap = a + row * a_row_stride + 16 * g;
    const uint8_t* as = a_scales + row * a_scale_stride + g;
    const uint8_t* bp = b + rc * k + 16 * g;
    const uint8_t* bs = b_scales + rc * (k / 32) + g;
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    for (uint64_t k0 = 0; k0 < k; k0 += 128) {
        const i32x8 a8 = load_halves(ap + k0), b8 = load_halves(bp + k0);
        const int sa = as[k0 / 32], sb = bs[k0 / 32];
        c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 0, 0, 0, sa, 0, sb);   // cbsz = blgp = 0: e4m3 x e4m3
    }
    float* o = out + (16ull * blockIdx.x + 4 * g) * 16 + rc;
    for (int i = 0; i < 4; ++i) o[16 * i] = c[i];
}

// 0, or -1 for arguments the kernel cannot take, or the HIP error of the launch.
// a + r * a_row_stride must be 16-byte aligned for every row (a and a_row_stride multiples of 16); b too.
extern "C" int mx_consume(const uint8_t* a, uint64_t a_row_stride, const uint8_t* a_scales, uint64_t a_scale_stride,
                          int m, uint64_t k, const uint8_t* b, const uint8_t* b_scales, float* out, void* stream) {
    if (!a || !a_scales || !b || !b_scales || !out) return -1;
    if (m <= 0 || m % 16 || k == 0 || k % 128) return -1;
    if (a_row_stride < k || a_row_stride % 16 || a_scale_stride < k / 32) return -1;
    if (reinterpret_cast<uintptr_t>(a) % 16 || reinterpret_cast<uintptr_t>(b) % 16) return -1;
    hipLaunchKernelGGL(k_mx_consume, dim3(m / 16), dim3(64), 0, static_cast<hipStream_t>(stream),
                       a, a_row_stride, a_scales, a_scale_stride, k, b, b_scales, out);
    return static_cast<int>(hipGetLastError());
}
