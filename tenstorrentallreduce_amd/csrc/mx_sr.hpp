// mx_sr.hpp — the stochastic rounding of the MXFP4 quantiser (allred.h, THE SR RULE), for the kernels that
// round the fp32 master values in the registers they already hold (mx4_sr_kernels.hip: k_ag_group_mxfp4_sr;
// adamw_mx4_sr_kernels.hip: k_adamw_ag_mxfp4_sr through adamw_body.hpp; mx4_2d_sr_kernels.hip:
// k_ag_group_mxfp4_2d_sr, on the column-wise rows): Philox4x32-10 and the integer conversion of one scaled value
// to an e2m1 nibble.
//
// The random word of an element depends on the seed, the step, the bucket's index in the caller's list and
// the element's position in the gathered row — on indices alone, so a kernel generates a tile's words while
// the tile's loads are in flight.  One Philox call yields the words of FOUR consecutive elements.
//
// No v_cvt_scalef32_sr_pk_fp4_f32 here: it takes one random word per PAIR and its rounding is not documented
// bit for bit; the rule is integer arithmetic, and this is the rule.
#pragma once

#include "allred.h"
#include "device.hpp"

namespace tsa {
namespace {

static_assert(sizeof(allred_mx_sr_state) == 16, "allred.h's layout");

// what is wave-uniform per call: the key and the counter's last word, read from device memory ONCE per wave
// (a wave-uniform address and only read: the compiler goes through the scalar cache)
struct SrCall {
    uint32_t k0, k1, step;
};
__device__ __forceinline__ SrCall sr_call(const allred_mx_sr_state* __restrict__ sr) {
    const uint64_t seed = sr->seed;
    return SrCall{(uint32_t)seed, (uint32_t)(seed >> 32), sr->step};
}

struct SrWords {
    uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1); ten rounds, the key bumped by
// the Weyl constants in front of rounds 2 .. 10.  c2 (the bucket), c3 (the step) and the key are wave-uniform
// in both kernels: round 1's second product and every key are scalar arithmetic after inlining.
__device__ __forceinline__ SrWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    return SrWords{{c0, c1, c2, c3}};
}

// the words of elements 4 g .. 4 g + 3 of a gathered row: g = (g_hi, g_lo), bucket the index in the CALLER's list
__device__ __forceinline__ SrWords sr_words(const SrCall& s, uint32_t g_lo, uint32_t g_hi, uint32_t bucket) {
    return philox4x32_10(g_lo, g_hi, bucket, s.step, s.k0, s.k1);
}

// One scaled value y (|y| < 8, or the block is special and the nibble is thrown away) and its word to the
// e2m1 nibble, the sign in bit 3.  a = |y|'s bits, r = the word's low 22 bits:
//   a >= 1.0   e2m1 keeps one mantissa bit there: bits 21:0 are what is dropped, a + r carries into bit 22
//              with probability (a & 0x3fffff) / 2^22, and (bits 31:22) - 0xFC is the code; a carry past 6
//              gives 8, which saturates to 7;
//   a <  1.0   the grid 0, 0.5, 1 is uniform: T = floor(|y| 2^23) — the exact product truncated by
//              v_cvt_u32_f32, which is the rule's shift of the mantissa, fp32 denormals giving 0 whether the
//              multiply keeps or flushes them —, and (T + r) >> 22 is the code.  The operand is clamped
//              below 1.0 so that the conversion's argument stays below 2^23 on the path not taken as well.
__device__ __forceinline__ uint32_t sr_code_fp4(float y, uint32_t word) {
    const uint32_t bits = __float_as_uint(y), a = bits & 0x7fffffffu, r = word & 0x3fffffu;
    const uint32_t over = ((a + r) >> 22) - 0xFCu;
    const uint32_t big = over < 7u ? over : 7u;
    const uint32_t below = a < 0x3f7fffffu ? a : 0x3f7fffffu;
    const uint32_t T = (uint32_t)(__uint_as_float(below) * 8388608.0f);
    const uint32_t small = (T + r) >> 22;
    return (a >= 0x3f800000u ? big : small) | ((bits >> 28) & 8u);
}

// four floats scaled by inv (ONE fp32 multiply each) into nibbles 0 .. 3 of the result, element i with word i
__device__ __forceinline__ uint32_t sr4_fp4(const f32x4& x, float inv, const SrWords& w) {
    uint32_t v = sr_code_fp4(x[0] * inv, w.w[0]);
    v |= sr_code_fp4(x[1] * inv, w.w[1]) << 4;
    v |= sr_code_fp4(x[2] * inv, w.w[2]) << 8;
    return v | sr_code_fp4(x[3] * inv, w.w[3]) << 12;
}

}  // namespace
}  // namespace tsa
