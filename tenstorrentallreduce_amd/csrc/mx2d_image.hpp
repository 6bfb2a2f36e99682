// mx2d_image.hpp — what the two kernels that quantise a patch of whole 32 x 32 squares in BOTH directions
// share (mx2d_kernels.hip: k_ag_group_mxfp8_2d; adamw_mx2d_kernels.hip: k_adamw_ag_mxfp8_2d): the LDS image
// of a patch's quantised bytes, the quantiser of 32 floats held by eight aligned lanes, and the scale store.
// Moved here from mx2d_kernels.hip unchanged (profiles/adamw_mx2d_isa.txt: its instances are identical).
#pragma once

#include "device.hpp"
#include "mx2d_span.hpp"
#include "mx_quant.hpp"

namespace tsa {
namespace {

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

}  // namespace
}  // namespace tsa
