// Device primitives shared by every conv kernel: the implicit-GEMM template (conv_igemm_kernel.h) and the fixed-shape kernels
// (conv_stem.hip, conv_block.hip, conv_s2.hip), which include only this header so that their compile stays light.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) char lds_char;

// two floats -> packed bf16 pair (lo | hi << 16) in ONE v_cvt_pk_bf16_f32 (RNE, NaN preserved)
__device__ __forceinline__ uint32_t f32x2_to_bf16x2(float lo, float hi)
{
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t));
}
// ---- 16-bit storage type of the 16-bit kernels: bf16 (8-bit significand) or, H16 = true, IEEE fp16 (11-bit significand; same MFMA
//      rate, v_mfma_f32_16x16x32_f16).  Values beyond fp16's range saturate at +-65504 on the way to memory. ----
// The saturation is the hardware's: the fp16 kernels set MODE.FP16_OVFL (fp16_saturating_mode below), under which a conversion that
// overflows yields +-65504 instead of an infinity -- two v_med3_f32 per stored pair less than clamping in fp32 first (that clamp was the
// 3-4 % fp16 cost against bf16).
__device__ __forceinline__ void fp16_saturating_mode() { __builtin_amdgcn_s_setreg((0 << 11) | (23 << 6) | 1, 1); }      // hwreg(HW_REG_MODE, 23, 1) = FP16_OVFL
template <bool H16> __device__ __forceinline__ uint32_t pack16x2(float lo, float hi)
{
    if constexpr (H16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{lo, hi}, f16x2_t));       // RNE, saturating (FP16_OVFL)
    else return f32x2_to_bf16x2(lo, hi);
}
template <bool H16> __device__ __forceinline__ float unpack16_lo(uint32_t w)
{
    if constexpr (H16) return (float)__builtin_bit_cast(f16x2_t, w)[0]; else return __builtin_bit_cast(float, w << 16);
}
template <bool H16> __device__ __forceinline__ float unpack16_hi(uint32_t w)
{
    if constexpr (H16) return (float)__builtin_bit_cast(f16x2_t, w)[1]; else return __builtin_bit_cast(float, w & 0xffff0000u);
}
template <bool H16> __device__ __forceinline__ f32x4 mma16(const bf16x8 a, const bf16x8 b, const f32x4 c)
{
    if constexpr (H16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// max(a, b) for finite operands without the sNaN-quieting v_max the compiler puts in front of fmaxf (one instruction, not two)
__device__ __forceinline__ float vmax_f32(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// The slope s of a slope-family activation (kernels.h): every conv epilogue evaluates max(v, v * s) -- linear 1, leaky 0.1, relie 0.01, relu 0.
// relu: the reference's x * (x > 0) (DN/activations.h:34) gives -0 for a negative x and so does max(v, 0 * v) = max(v, -0); +-0 and NaN pass
// through in both; +inf: 0 * inf is NaN and v_max returns its other operand, +inf, as the reference does.  -inf alone differs: the reference's
// -inf * 0 is NaN, max(-inf, NaN) is -inf.  Any other code (the planner never hands one to a conv) is linear.
__host__ __device__ __forceinline__ float act_slope(int act) { return act == ACT_LEAKY ? 0.1f : act == ACT_RELU ? 0.f : act == ACT_RELIE ? 0.01f : 1.f; }
// acc + bias, activation (slope 0.1: leaky as max(v, 0.1 v); slope 1: linear), rounded to the storage type: four channels as two packed words
template <bool H16> __device__ __forceinline__ uint2 leaky_pack4(const f32x4 acc, const f32x4 bias, const float slope)
{
    const f32x4 v = acc + bias;
    const f32x4 t = v * slope;
    return uint2{pack16x2<H16>(vmax_f32(v[0], t[0]), vmax_f32(v[1], t[1])), pack16x2<H16>(vmax_f32(v[2], t[2]), vmax_f32(v[3], t[3]))};
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void block_barrier() { asm volatile("s_barrier" ::: "memory"); }
// immediate of __builtin_amdgcn_s_waitcnt (gfx9: vmcnt in bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8); expcnt is never waited for,
// vmcnt 63 does not wait for vector memory
constexpr int waitcnt_imm(int vmcnt, int lgkmcnt) { return (vmcnt & 15) | ((vmcnt >> 4) << 14) | (7 << 4) | (lgkmcnt << 8); }

// buffer descriptor based at `p` covering 2 GiB: an offset at or beyond 0x80000000 reads zeros and drops a store
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *p) { return __builtin_amdgcn_make_buffer_rsrc((void *)p, 0, 0x80000000u, 0x00020000); }
