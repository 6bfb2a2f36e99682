// mx_quant.hpp — the device helpers of the MXFP8 quantisation, shared by the two kernels that write
// OCP MX operands (mx_kernels.hip: k_ag_group_mxfp8; adamw_mx_kernels.hip: k_adamw_ag_mxfp8 through
// adamw_body.hpp): the integer amax across lanes, the clamp and the conversion to e4m3fn — and of
// the MXFP4 all-gather (mx4_kernels.hip: k_ag_group_mxfp4): the conversion to e2m1 nibbles, and the
// side table it shares with mx_kernels.hip.
#pragma once

#include "allred.h"
#include "device.hpp"

namespace tsa {
namespace {

// The by-value side table of the two all-gathers that take an allred_mx_bucket_f32 list (mx_kernels.hip,
// mx4_kernels.hip), next to GroupSpan: entry i for bucket i of the launch, block b of the bucket at
// shard + b * stride floats, rank r's scale row at scales + r * scale_stride bytes.  Two more words per
// entry than GroupShardF32, hence 32 entries: 2064 + 1024 = 3088 bytes of kernel arguments.
struct MxShard {           // 32 bytes
    const float* shard;
    uint64_t stride;       // floats
    uint8_t* scales;
    uint64_t scale_stride; // bytes
};
struct MxShards {
    MxShard s[ALLRED_MX_GROUP_MAX];   // entries past the last bucket: zero
};
static_assert(sizeof(MxShard) == 32 && sizeof(MxShards) == 32 * ALLRED_MX_GROUP_MAX, "the kernel-argument layout");

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

// The MXFP4 tail (mx4_kernels.hip).  y0, y1 clamped to [-6, 6] (v_med3_f32, as cvt2 clamps) and rounded
// to e2m1 into byte SEL of `old`, y0 in bits 3:0 and y1 in bits 7:4: v_cvt_scalef32_pk_fp4_f32 with
// the scale 1.0 — IEEE RNE onto 0, 0.5, 1, 1.5, 2, 3, 4, 6 (ties to the even code), the sign kept on
// a zero result.  What it does above 6, and its own scaling, are never asked of it.
template <int SEL>
__device__ __forceinline__ uint32_t cvt2_fp4(float y0, float y1, uint32_t old) {
    y0 = __builtin_amdgcn_fmed3f(y0, -6.0f, 6.0f);
    y1 = __builtin_amdgcn_fmed3f(y1, -6.0f, 6.0f);
    return (uint32_t)__builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, y0, y1, 1.0f, SEL);
}

// eight floats scaled by inv (ONE fp32 multiply each) into the eight nibbles of a word, element i in
// nibble i: byte i / 2, the even element in the low nibble
__device__ __forceinline__ uint32_t cvt8_fp4(const f32x4& a, const f32x4& b, float inv) {
    uint32_t v = cvt2_fp4<0>(a[0] * inv, a[1] * inv, 0u);
    v = cvt2_fp4<1>(a[2] * inv, a[3] * inv, v);
    v = cvt2_fp4<2>(b[0] * inv, b[1] * inv, v);
    return cvt2_fp4<3>(b[2] * inv, b[3] * inv, v);
}

// the largest abs bit pattern of four floats
__device__ __forceinline__ uint32_t amax4(const f32x4& a) {
    return umax(umax(abs_bits(a[0]), abs_bits(a[1])), umax(abs_bits(a[2]), abs_bits(a[3])));
}

// the value lane l of this wave holds in x (l a constant)
__device__ __forceinline__ uint32_t lane_of(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }

}  // namespace
}  // namespace tsa
