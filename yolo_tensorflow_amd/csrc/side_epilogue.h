// The store of the side convs' MFMA kernels (deconv.hip, gconv.hip, xconv.hip; SideConvArgs in kernels.h).  All three keep the filters as
// the A operand and the pixels as the B operand, so a lane's accumulator holds its pixel (lane & 15) and four consecutive channels
// ((lane >> 4) * 4 + j): one 16-byte (fp32) or 8-byte (16-bit) piece of the output.  The caller applies its affine step (acc + bias, or
// float(acc) * scale + bias) and skips the pieces at or past Cstore; the activation and the encoders are here.
#pragma once
#include "kernels.h"
#include "device_common.h"

// two floats -> one packed pair of `dt` (DT_F16 or DT_BF16), round to nearest even.  fp16 saturates at +-65504 as the other fp16 stores of the
// library do; these kernels do not set FP16_OVFL, so the clamp is in fp32.  bf16: the one packed conversion (NaN kept)
__device__ __forceinline__ uint32_t side_pack2(int dt, float lo, float hi)
{
    if (dt == DT_F16) {
        lo = __builtin_amdgcn_fmed3f(lo, -65504.f, 65504.f); hi = __builtin_amdgcn_fmed3f(hi, -65504.f, 65504.f);
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{lo, hi}, f16x2_t));
    }
    return f32x2_to_bf16x2(lo, hi);
}

// v[0..3]: the finished values of four consecutive channels of one pixel, which begin at element `at` of `out` (a multiple of 4).
// max(v, v * slope), then the store in `out_dt`.  (A kernel whose 16-bit type is a template parameter passes a constant for it.)
__device__ __forceinline__ void side_store4(void *out, long at, int out_dt, float slope, const float (&v)[4])
{
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = fmaxf(v[j], v[j] * slope);
    if (out_dt == DT_F32) *(float4 *)((float *)out + at) = float4{r[0], r[1], r[2], r[3]};
    else *(uint2 *)((uint16_t *)out + at) = uint2{side_pack2(out_dt, r[0], r[1]), side_pack2(out_dt, r[2], r[3])};
}
