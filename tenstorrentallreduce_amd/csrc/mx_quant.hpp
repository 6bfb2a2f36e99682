// mx_quant.hpp — the device helpers of the MXFP8 quantisation, shared by the two kernels that write
// OCP MX operands (mx_kernels.hip: k_ag_group_mxfp8; adamw_mx_kernels.hip: k_adamw_ag_mxfp8 through
// adamw_body.hpp): the integer amax across lanes, the clamp and the conversion to e4m3fn.
#pragma once

#include "device.hpp"

namespace tsa {
namespace {

// max(x, the x of the lane a DPP control names), as unsigned integers: add_dpp's idiom (device.hpp)
template <int CTRL>
__device__ __forceinline__ uint32_t max_dpp(uint32_t x) {
    const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
    return x > y ? x : y;
}

__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// y clamped to [-448, 448] (v_med3_f32: a finite y in range, its sign and a denormal included, passes
// unchanged) and two of them rounded to e4m3fn into bytes 0-1 (HI = false) or 2-3 of `old`:
// v_cvt_pk_fp8_f32, which is OCP e4m3fn on gfx950 — IEEE RNE, subnormals multiples of 2^-9, the sign
// kept on a zero result.  What it does above 448 is never asked of it.
template <bool HI>
__device__ __forceinline__ uint32_t cvt2(float y0, float y1, uint32_t old) {
    y0 = __builtin_amdgcn_fmed3f(y0, -448.0f, 448.0f);
    y1 = __builtin_amdgcn_fmed3f(y1, -448.0f, 448.0f);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, (int)old, HI);
}

// the value lane l of this wave holds in x (l a constant)
__device__ __forceinline__ uint32_t lane_of(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }

}  // namespace
}  // namespace tsa
