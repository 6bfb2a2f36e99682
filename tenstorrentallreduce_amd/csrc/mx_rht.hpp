// mx_rht.hpp — the random Hadamard rotation of an MX block (allred.h, THE ROTATION), for the kernels that
// rotate the fp32 master values in the registers they already hold, in front of the MXFP4 quantiser
// (mx4_rht_kernels.hip: k_ag_group_mxfp4_rht; adamw_mx4_rht_kernels.hip: k_adamw_ag_mxfp4_rht through
// adamw_body.hpp; the SR kernels, mx4_2d_sr_kernels.hip's column phase among them).
//
// The rule fixes every fp32 operation and its order: the sign flips, then the five butterfly stages
// h = 1, 2, 4, 8, 16 — (x[i], x[i + h]) <- (x[i] + x[i + h], x[i] - x[i + h]) for (i & h) == 0 —, then ONE
// multiply by 2^-2.5.  A lane holds N consecutive elements of a block (N = 16 or 4), so the stages h < N are
// register arithmetic and every stage h >= N pairs this lane with the lane h / N away.  Across lanes the lane
// with the lower elements computes own + partner and the other one partner - own, written as
// partner + (own ^ sign bit): the same IEEE sum, so both are ONE v_add_f32 whose first operand comes through
// DPP.  No matrix instruction: the order of the additions is the contract, an MFMA's is not documented.
// The build keeps denormals and has -ffp-contract=off; nothing here can fuse anyway (no multiply feeds an add).
#pragma once

#include "device.hpp"

namespace tsa {
namespace {

constexpr uint32_t kRhtNormBits = 0x3E3504F3u;   // 2^-2.5 rounded to nearest

__device__ __forceinline__ float flip(float x, uint32_t sign) { return __uint_as_float(__float_as_uint(x) ^ sign); }

// What a lane prepares ONCE, outside its tile loop: the sign-bit masks of its N elements — bit (N * pos + e) of
// sign_mask moved to bit 31, pos the lane's place among the 32 / N lanes of a block — and, for the cross-lane
// stage over lane bit k, the sign bit where the lane holds the upper elements of the pair (it subtracts).
template <int N>
struct RhtLane {
    uint32_t sign[N];
    uint32_t upper[5];   // indexed by k = log2 of the lane distance; the kernels use k < log2(32 / N)
};
template <int N>
__device__ __forceinline__ RhtLane<N> rht_lane(uint32_t sign_mask, int pos) {
    RhtLane<N> r;
    const uint32_t mine = sign_mask >> (N * pos);
#pragma unroll
    for (int e = 0; e < N; ++e) r.sign[e] = (mine >> e) << 31;
#pragma unroll
    for (int k = 0; k < 5; ++k) r.upper[k] = ((uint32_t)pos >> k) << 31;
    return r;
}

// the signs and the stages h = 1 .. N / 2 on the lane's own elements, in the rule's order
template <int N>
__device__ __forceinline__ void rht_own(float (&x)[N], const RhtLane<N>& r) {
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = flip(x[e], r.sign[e]);
#pragma unroll
    for (int h = 1; h < N; h *= 2) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (i & h) continue;
            const float a = x[i], b = x[i + h];
            x[i] = a + b;
            x[i + h] = a - b;
        }
    }
}

// one cross-lane stage: `partner` is the paired lane's x (the caller's DPP), `upper` this lane's mask for the stage
__device__ __forceinline__ float rht_pair(float partner, float x, uint32_t upper) { return partner + flip(x, upper); }

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}

// the closing multiply: ONE v_mul_f32, its own rounding (the quantiser's multiply by 2^-X stays a second one)
__device__ __forceinline__ float rht_norm(float x) { return x * __uint_as_float(kRhtNormBits); }

}  // namespace
}  // namespace tsa
