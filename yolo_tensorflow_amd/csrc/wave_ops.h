// Wave64 collectives shared by the post-processing, classifier and tree kernels (post_ops.hip, cls_ops.hip, tree_ops.hip).  Every lane
// returns the result; the butterfly adds / compares the same two operands in both lanes of a pair, so all lanes hold the same bits.
#pragma once
#include <hip/hip_runtime.h>

// One more class score of a box, taken in ascending class order: the strict > keeps the first maximum (argmax's choice)
__device__ __forceinline__ void first_max(float &best, int &label, float sc, int k)
{
    if (sc > best) { best = sc; label = k; }
}
// wave-wide (value, first index) arg-max over lanes; every lane returns the result
__device__ __forceinline__ void wave_argmax(float &v, int &idx)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float ov = __shfl_xor(v, off);
        int oi = __shfl_xor(idx, off);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}
__device__ __forceinline__ float wave_max(float m)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}
__device__ __forceinline__ float wave_sum(float s)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
// the order of classify()'s stable sort by -prob: larger probability first, equal probabilities by ascending index; index -1: nothing
__device__ __forceinline__ bool ranks_before(float p2, int i2, float p1, int i1) { return i2 >= 0 && (i1 < 0 || p2 > p1 || (p2 == p1 && i2 < i1)); }
// block-wide best (p, i) in that order over any whole number of waves up to 16; every thread returns it; red_p / red_i: one slot per wave
__device__ __forceinline__ void block_best(float &p, int &i, float *red_p, int *red_i)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float p2 = __shfl_xor(p, o, 64); const int i2 = __shfl_xor(i, o, 64);
        if (ranks_before(p2, i2, p, i)) { p = p2; i = i2; }
    }
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red_p[threadIdx.x >> 6] = p; red_i[threadIdx.x >> 6] = i; }
    __syncthreads();
    p = red_p[0]; i = red_i[0];
    for (int w = 1; w < nw; ++w) if (ranks_before(red_p[w], red_i[w], p, i)) { p = red_p[w]; i = red_i[w]; }
}
