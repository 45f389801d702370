// Element access of the memory-bound operators (ew_ops.hip, map_ops.hip): one 8-channel granule (16 B of a 16-bit type, 32 B of fp32) or one
// element of a tensor stored as bf16 / fp16 / fp32 / e4m3, as floats; WITH_DT binds T to the element type of a DT_* code.
#pragma once
#include "kernels.h"
#include "device_common.h"

template <typename T> struct Elt;
template <> struct Elt<bf16_t> {
    static __device__ __forceinline__ void load8(const bf16_t *p, float *v)
    {
        uint4 u = *(const uint4 *)p;
        uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __builtin_bit_cast(float, w[i] << 16);
            v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ uint32_t cvt(float f)
    {
        __bf16 b = (__bf16)f;
        return (uint32_t)__builtin_bit_cast(uint16_t, b);
    }
    static __device__ __forceinline__ void store8(bf16_t *p, const float *v)
    {
        uint4 u;
        u.x = cvt(v[0]) | (cvt(v[1]) << 16); u.y = cvt(v[2]) | (cvt(v[3]) << 16);
        u.z = cvt(v[4]) | (cvt(v[5]) << 16); u.w = cvt(v[6]) | (cvt(v[7]) << 16);
        *(uint4 *)p = u;
    }
    static __device__ __forceinline__ float load1(const bf16_t *p) { return __builtin_bit_cast(float, (uint32_t)(*p) << 16); }
    static __device__ __forceinline__ void store1(bf16_t *p, float f) { *p = (bf16_t)cvt(f); }
};
template <> struct Elt<f16_t> {       // IEEE binary16: decode exact, encode round-to-nearest-even, saturating at +-65504 (as the conv epilogues do)
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ void load8(const f16_t *p, float *v)
    {
        uint4 u = *(const uint4 *)p;
        uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { const h2 h = __builtin_bit_cast(h2, w[i]); v[2 * i] = (float)h[0]; v[2 * i + 1] = (float)h[1]; }
    }
    static __device__ __forceinline__ uint32_t pk(float a, float b)
    {
        a = __builtin_amdgcn_fmed3f(a, -65504.f, 65504.f); b = __builtin_amdgcn_fmed3f(b, -65504.f, 65504.f);
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{a, b}, h2));
    }
    static __device__ __forceinline__ void store8(f16_t *p, const float *v)
    {
        *(uint4 *)p = uint4{pk(v[0], v[1]), pk(v[2], v[3]), pk(v[4], v[5]), pk(v[6], v[7])};
    }
    static __device__ __forceinline__ float load1(const f16_t *p) { return (float)__builtin_bit_cast(_Float16, p->b); }
    static __device__ __forceinline__ void store1(f16_t *p, float f) { p->b = (uint16_t)(pk(f, 0.f) & 0xffffu); }
};
template <> struct Elt<float> {
    static __device__ __forceinline__ void load8(const float *p, float *v)
    {
        float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void store8(float *p, const float *v)
    {
        *(float4 *)p = float4{v[0], v[1], v[2], v[3]};
        *(float4 *)(p + 4) = float4{v[4], v[5], v[6], v[7]};
    }
    static __device__ __forceinline__ float load1(const float *p) { return *p; }
    static __device__ __forceinline__ void store1(float *p, float f) { *p = f; }
};

template <> struct Elt<fp8_t> {      // OCP e4m3: decode is exact, encode is round-to-nearest-even with saturation at +-448
    template <bool HI> static __device__ __forceinline__ uint32_t enc2(float a, float b, uint32_t old)
    {
        a = __builtin_amdgcn_fmed3f(a, -FP8_MAX, FP8_MAX); b = __builtin_amdgcn_fmed3f(b, -FP8_MAX, FP8_MAX);
        return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, HI);
    }
    static __device__ __forceinline__ void load8(const fp8_t *p, float *v)
    {
        uint2 u = *(const uint2 *)p;
        v[0] = __builtin_amdgcn_cvt_f32_fp8((int)u.x, 0); v[1] = __builtin_amdgcn_cvt_f32_fp8((int)u.x, 1);
        v[2] = __builtin_amdgcn_cvt_f32_fp8((int)u.x, 2); v[3] = __builtin_amdgcn_cvt_f32_fp8((int)u.x, 3);
        v[4] = __builtin_amdgcn_cvt_f32_fp8((int)u.y, 0); v[5] = __builtin_amdgcn_cvt_f32_fp8((int)u.y, 1);
        v[6] = __builtin_amdgcn_cvt_f32_fp8((int)u.y, 2); v[7] = __builtin_amdgcn_cvt_f32_fp8((int)u.y, 3);
    }
    static __device__ __forceinline__ void store8(fp8_t *p, const float *v)
    {
        uint2 u;
        u.x = enc2<true>(v[2], v[3], enc2<false>(v[0], v[1], 0));
        u.y = enc2<true>(v[6], v[7], enc2<false>(v[4], v[5], 0));
        *(uint2 *)p = u;
    }
    static __device__ __forceinline__ float load1(const fp8_t *p) { return __builtin_amdgcn_cvt_f32_fp8((int)p->b, 0); }
    static __device__ __forceinline__ void store1(fp8_t *p, float f) { p->b = (uint8_t)(enc2<false>(f, 0.f, 0) & 0xff); }
};

// run `stmt` with T bound to the element type of `dt`
#define WITH_DT(dt, ...)                                                         \
    do {                                                                         \
        if ((dt) == DT_F32) { typedef float T; __VA_ARGS__; }                    \
        else if ((dt) == DT_FP8) { typedef fp8_t T; __VA_ARGS__; }               \
        else if ((dt) == DT_F16) { typedef f16_t T; __VA_ARGS__; }               \
        else { typedef bf16_t T; __VA_ARGS__; }                                  \
    } while (0)

static inline dim3 grid_for(size_t n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }
