// Vector-input networks and sequences: the rows a vector network reads -- from fp32 vectors, from tokens -- and darknet's sampler,
// which closes the loop of a generation on the device: the token it draws from one step's [softmax] row is the next step's one-hot input row.
// A step of yolo_sequence is a sequence of ordinary launches; nothing here waits on another workgroup.
#include "elt.h"

namespace {

constexpr int SQ_NT = 256;

// ---- x fp32 [n][len] -> rows [n][row_stride] of T, zero behind len.  One thread per 8-element granule: grid (granules / SQ_NT, n) ----
template <typename T> __global__ __launch_bounds__(SQ_NT) void k_vector_in(const float *x, int len, T *rows, int row_stride)
{
    const int g = blockIdx.x * SQ_NT + threadIdx.x, b = blockIdx.y;
    if (g * 8 >= row_stride) return;
    const float *src = x + (size_t)b * len;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = g * 8 + j < len ? src[g * 8 + j] : 0.f;
    Elt<T>::store8(rows + (size_t)b * row_stride + (size_t)g * 8, v);
}

// the granule g of a one-hot row: 1 at `tok`, 0 elsewhere (tok outside the row: zeros)
template <typename T> __device__ __forceinline__ void one_hot_granule(T *row, int g, int tok)
{
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = g * 8 + j == tok ? 1.f : 0.f;
    Elt<T>::store8(row + (size_t)g * 8, v);
}

// ---- tokens [n] -> one-hot rows, each granule of a row written once ----
template <typename T> __global__ __launch_bounds__(SQ_NT) void k_token_in(const int32_t *tokens, int len, T *rows, int row_stride)
{
    const int g = blockIdx.x * SQ_NT + threadIdx.x, b = blockIdx.y;
    if (g * 8 >= row_stride) return;
    const int t = tokens[b];
    one_hot_granule(rows + (size_t)b * row_stride, g, t >= 0 && t < len ? t : -1);
}

// ---- the sampler: one workgroup per stream, the row staged in LDS once (the layout of k_softmax_topk); lane 0 does the serial part, in the
//      reference's order: a parallel prefix would round differently.  Every product and difference is rounded on its own (no fma): the reference
//      stores the scaled value before it subtracts it ----
template <typename T> __global__ __launch_bounds__(SQ_NT) void k_sample(const float *probs, int p_stride, int len, const float *uniforms, float clip,
                                                                        int32_t *tokens_out, T *next_rows, int row_stride, float *probs_out)
{
    __shared__ float v[CLS_SOFTMAX_MAX];
    __shared__ int s_tok;
    const int b = blockIdx.x;
    const float *src = probs + (size_t)b * p_stride;
    for (int i = threadIdx.x; i < len; i += SQ_NT) { const float p = src[i]; v[i] = p; if (probs_out) probs_out[(size_t)b * len + i] = p; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        for (int i = 0; i < len; ++i) { float p = v[i]; if (p < clip) p = 0.f; v[i] = p; sum = __fadd_rn(sum, p); }      // rnn.c:290-292, sum_array
        const float scale = (float)(1. / (double)sum);                                                                   // scale_array(a, n, 1./sum)
        float r = uniforms[b];
        int tok = len - 1;
        for (int i = 0; i < len; ++i) {
            r = __fsub_rn(r, __fmul_rn(v[i], scale));
            if (r <= 0.f) { tok = i; break; }
        }
        tokens_out[b] = tok;
        s_tok = tok;
    }
    __syncthreads();
    if (!next_rows) return;
    const int tok = s_tok;
    for (int g = threadIdx.x; g * 8 < row_stride; g += SQ_NT) one_hot_granule(next_rows + (size_t)b * row_stride, g, tok);
}

bool rows_ok(const void *rows, int n, int len, int row_stride, int dt)
{
    return rows && n >= 1 && n <= 65535 && len >= 1 && row_stride >= len && row_stride % 8 == 0 && ((uintptr_t)rows & 15) == 0 && (dt == DT_BF16 || dt == DT_F16 || dt == DT_F32);
}

}  // namespace

hipError_t launch_vector_in(const float *x, int n, int len, void *rows, int row_stride, int dt, hipStream_t s)
{
    if (!x || !rows_ok(rows, n, len, row_stride, dt)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((row_stride / 8 + SQ_NT - 1) / SQ_NT), (unsigned)n);
    if (dt == DT_F32) k_vector_in<float><<<grid, SQ_NT, 0, s>>>(x, len, (float *)rows, row_stride);
    else if (dt == DT_F16) k_vector_in<f16_t><<<grid, SQ_NT, 0, s>>>(x, len, (f16_t *)rows, row_stride);
    else k_vector_in<bf16_t><<<grid, SQ_NT, 0, s>>>(x, len, (bf16_t *)rows, row_stride);
    return hipGetLastError();
}

hipError_t launch_token_in(const int32_t *tokens, int n, int len, void *rows, int row_stride, int dt, hipStream_t s)
{
    if (!tokens || !rows_ok(rows, n, len, row_stride, dt)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((row_stride / 8 + SQ_NT - 1) / SQ_NT), (unsigned)n);
    if (dt == DT_F32) k_token_in<float><<<grid, SQ_NT, 0, s>>>(tokens, len, (float *)rows, row_stride);
    else if (dt == DT_F16) k_token_in<f16_t><<<grid, SQ_NT, 0, s>>>(tokens, len, (f16_t *)rows, row_stride);
    else k_token_in<bf16_t><<<grid, SQ_NT, 0, s>>>(tokens, len, (bf16_t *)rows, row_stride);
    return hipGetLastError();
}

hipError_t launch_sample(const SampleArgs &a, hipStream_t s)
{
    if (!a.probs || !a.uniforms || !a.tokens_out || a.n < 1 || a.len < 1 || a.len > CLS_SOFTMAX_MAX || a.p_stride < a.len) return hipErrorInvalidValue;
    if (a.next_rows && !rows_ok(a.next_rows, a.n, a.len, a.row_stride, a.dt)) return hipErrorInvalidValue;
    if (!a.next_rows || a.dt == DT_F32) k_sample<float><<<a.n, SQ_NT, 0, s>>>(a.probs, a.p_stride, a.len, a.uniforms, a.clip, a.tokens_out, (float *)a.next_rows, a.row_stride, a.probs_out);
    else if (a.dt == DT_F16) k_sample<f16_t><<<a.n, SQ_NT, 0, s>>>(a.probs, a.p_stride, a.len, a.uniforms, a.clip, a.tokens_out, (f16_t *)a.next_rows, a.row_stride, a.probs_out);
    else k_sample<bf16_t><<<a.n, SQ_NT, 0, s>>>(a.probs, a.p_stride, a.len, a.uniforms, a.clip, a.tokens_out, (bf16_t *)a.next_rows, a.row_stride, a.probs_out);
    return hipGetLastError();
}
