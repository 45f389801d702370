// The small layers of a dense-prediction network -- [l2norm], darknet's [upsample] with any stride and a scale -- and the outputs of a
// map network: per-pixel labels of the map, labels at every source image's own size, the planar copy darknet's net->output holds.
// Memory-bound, NHWC; compiled with -ffp-contract=off like ew_ops.hip.
#include "kernels.h"
#include "elt.h"
#include "wave_ops.h"
#include <math.h>

// ---- [l2norm] (DN/blas.c:126-144 l2normalize_cpu): one wave per pixel, the lanes stride over the channels; fp32 sum of squares, one
//      wave reduction, sqrtf, then x / norm (a division, and no epsilon: an all-zero pixel is 0 / 0 = NaN as in the reference).  The
//      channels C .. of the last granule are written as zeros. ----
// (the fp16 encoder clamps to +-65504 on the way to memory, which would turn the NaN into a number: it is written as NaN itself)
template <typename T> __device__ __forceinline__ void store1_keep_nan(T *p, float v) { Elt<T>::store1(p, v); }
template <> __device__ __forceinline__ void store1_keep_nan<f16_t>(f16_t *p, float v) { if (v != v) p->b = 0x7e00; else Elt<f16_t>::store1(p, v); }
template <typename T>
__global__ __launch_bounds__(256) void k_l2norm(const T *in, int is, T *out, int os, size_t npix, int C, int Cw)
{
    const size_t p = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;          // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const T *x = in + p * is; T *y = out + p * os;
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) { const float v = Elt<T>::load1(x + c); sum += v * v; }
    const float norm = sqrtf(wave_sum(sum));
    for (int c = lane; c < Cw; c += 64) store1_keep_nan<T>(y + c, c < C ? Elt<T>::load1(x + c) / norm : 0.f);
}
hipError_t launch_l2norm(const TView &in, const TView &out, hipStream_t s)
{
    if (in.dt != out.dt || in.dt == DT_FP8 || in.c != out.c || in.c < 1 || in.stride < in.c || out.stride < out.c) return hipErrorInvalidValue;
    const size_t npix = (size_t)in.n * in.h * in.w;
    const int cw = std::min(out.stride, (out.c + 7) / 8 * 8);
    WITH_DT(in.dt, hipLaunchKernelGGL(k_l2norm<T>, dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, npix, in.c, cw));
    return hipGetLastError();
}

// ---- [normalization] / [lrn] (DN/normalization_layer.c:66-95): local response normalisation over the channels of a pixel.
//      The reference keeps a RUNNING sum over the channels.  With sq[j] = x[j]^2, h = size / 2, lo = (size - 1) / 2:
//        norms[0] = kappa + alpha * (sq[0] + .. + sq[h - 1])                          (:80-83, the initial loop stops BEFORE channel h)
//        norms[k] = norms[k - 1] - alpha * sq[k - lo - 1] + alpha * sq[k + h]         (:85-91, each term only where its index is a channel)
//      The loop over k adds the channels h + 1, h + 2, ..: channel h is never added, but it is subtracted once the window has passed it
//      (k - lo - 1 == h).  Against the textbook window W(k) = sum of sq[j] over max(0, k - lo) <= j <= min(C - 1, k + h): while the window
//      holds channel h the running sum lacks it, and afterwards the running sum has lost it once more than the window -- either way, for
//      EVERY k,
//        norms[k] = kappa + alpha * (W(k) - g),   g = sq[h] where h < C, 0 where h == C (no such channel),   out[k] = x[k] * norms[k]^(-beta)
//      (pow_cpu + mul_cpu, :93-94).  A negative norms[k] is NaN there (pow of a negative base) and here; nothing is clamped.  size / 2 > C makes
//      the reference's initial loop read past the image: the planner refuses it.
//      One thread per 8-channel granule, consecutive lanes along a pixel's channels (then along the pixels): it squares its own granule and its
//      two neighbours' (16-byte loads the neighbouring lanes issue as well: one trip to HBM), which hold every window of a size up to
//      LRN_MAX_SIZE = 17 (h and lo at most 8).  W(k) is the direct sum of the window's squares in ascending channel order, fp32 -- a difference of
//      prefix sums would cancel.  The window offsets are wave-uniform, so the loop over them branches on scalars and indexes registers with
//      constants.  x^(-0.75), the default, is rsq(n) * sqrt(rsq(n)); any other beta is exp2(-beta * log2(n)) on the hardware's
//      log2 / exp2 (docs/NOTEBOOK.md holds the measured error of both).  Channels C .. of the last granule are stored as zeros. ----
template <typename T> __device__ __forceinline__ void store8_keep_nan(T *p, const float *v) { Elt<T>::store8(p, v); }
template <> __device__ __forceinline__ void store8_keep_nan<f16_t>(f16_t *p, const float *v)
{
    Elt<f16_t>::store8(p, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) if (v[i] != v[i]) p[i].b = 0x7e00;          // (the encoder's clamp turns a NaN into -65504: see store1_keep_nan)
}
template <typename T>
__global__ __launch_bounds__(256) void k_lrn(const T *in, int is, T *out, int os, size_t npix, int C, int c8, int lo, int h, float alpha, float beta, float kappa)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    const size_t p = idx / c8; const int g = (int)(idx - p * c8);
    const T *x = in + p * is;
    float s[24], v[8];          // squares of the channels 8 (g - 1) .. 8 (g + 2), zero where there is no channel; v: this granule's values
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int gq = g + q - 1;
        float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (gq >= 0 && gq * 8 < C) Elt<T>::load8(x + gq * 8, t);
#pragma unroll
        for (int i = 0; i < 8; ++i) { if (q == 1) v[i] = t[i]; s[q * 8 + i] = gq * 8 + i < C ? t[i] * t[i] : 0.f; }
    }
    float ghost = 0.f;
    if (h < C) { ghost = Elt<T>::load1(x + h); ghost *= ghost; }
    float w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int d = -8; d <= 8; ++d)
        if (d >= -lo && d <= h) {          // (uniform)
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] += s[8 + i + d];
        }
    float r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float n = kappa + alpha * (w[i] - ghost);
        float pw;
        if (beta == 0.75f) { const float t = __builtin_amdgcn_rsqf(n); pw = t * __builtin_amdgcn_sqrtf(t); }
        else pw = __builtin_amdgcn_exp2f(-beta * __builtin_amdgcn_logf(n));
        r[i] = g * 8 + i < C ? v[i] * pw : 0.f;
    }
    store8_keep_nan<T>(out + p * os + g * 8, r);
}
hipError_t launch_lrn(const TView &in, const TView &out, int size, float alpha, float beta, float kappa, hipStream_t s)
{
    const int c8 = (in.c + 7) / 8;
    if (in.dt != out.dt || in.dt == DT_FP8 || in.c != out.c || in.c < 1 || out.h != in.h || out.w != in.w || size < 1 || size > LRN_MAX_SIZE || size / 2 > in.c ||
        in.stride < c8 * 8 || out.stride < c8 * 8 || in.stride % 8 || out.stride % 8) return hipErrorInvalidValue;
    const size_t npix = (size_t)in.n * in.h * in.w;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_lrn<T>, grid_for(npix * c8), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, npix, in.c, c8, (size - 1) / 2, size / 2, alpha, beta, kappa));
    return hipGetLastError();
}

// ---- [crop] at inference (DN/crop_layer.c:67-102 with net.train == 0): the centred crop_h x crop_w window, dh = (H - crop_h) / 2, dw = (W - crop_w) / 2,
//      out[y][x][c] = in[y + dh][x + dw][c] * 2 - 1 (a product, then a sum: fp32, no contraction), or the plain copy with noadjust=1.  One thread
//      per granule; the channels C .. of the last granule stay zeros, whatever the adjustment does to a zero ----
template <typename T>
__global__ void k_crop(const T *in, int is, T *out, int os, int n, int h, int w, int ho, int wo, int dh, int dw, int C, int c8, int adjust)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * ho * wo * c8) return;
    const int g = (int)(idx % c8); size_t p = idx / c8;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho), b = (int)(p / ho);
    float r[8];
    Elt<T>::load8(in + (((size_t)b * h + oy + dh) * w + ox + dw) * is + g * 8, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = g * 8 + i < C ? (adjust ? r[i] * 2.f + -1.f : r[i]) : 0.f;
    Elt<T>::store8(out + (((size_t)b * ho + oy) * wo + ox) * os + g * 8, r);
}
hipError_t launch_crop(const TView &in, const TView &out, int adjust, hipStream_t s)
{
    const int c8 = (out.c + 7) / 8;          // (the network input's view counts its 8 padded channels: the layer's own count is the output's)
    if (in.dt != out.dt || in.dt == DT_FP8 || out.c < 1 || in.c < out.c || out.h < 1 || out.w < 1 || out.h > in.h || out.w > in.w || in.n != out.n ||
        in.stride < c8 * 8 || out.stride < c8 * 8 || in.stride % 8 || out.stride % 8) return hipErrorInvalidValue;
    const size_t total = (size_t)in.n * out.h * out.w * c8;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_crop<T>, grid_for(total), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, out.h, out.w,
                                      (in.h - out.h) / 2, (in.w - out.w) / 2, out.c, c8, adjust));
    return hipGetLastError();
}

// ---- darknet's [upsample] (DN/blas.c:334-349 upsample_cpu, forward): out[y][x] = scale * in[y / stride][x / stride] ----
template <typename T>
__global__ void k_upsample_nearest(const T *in, int is, T *out, int os, int n, int h, int w, int c8, int stride, float scale)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ho = h * stride, wo = w * stride;
    if (idx >= (size_t)n * ho * wo * c8) return;
    const int g = (int)(idx % c8); size_t p = idx / c8;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho), b = (int)(p / ho);
    float r[8];
    Elt<T>::load8(in + (((size_t)b * h + oy / stride) * w + ox / stride) * is + g * 8, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = scale * r[i];
    Elt<T>::store8(out + (((size_t)b * ho + oy) * wo + ox) * os + g * 8, r);
}
hipError_t launch_upsample_nearest(const TView &in, const TView &out, int stride, float scale, hipStream_t s)
{
    const int c8 = (in.c + 7) / 8;
    if (in.dt != out.dt || in.dt == DT_FP8 || stride < 1 || out.h != in.h * stride || out.w != in.w * stride || in.stride < c8 * 8 || out.stride < c8 * 8 ||
        in.stride % 8 || out.stride % 8) return hipErrorInvalidValue;
    const size_t total = (size_t)in.n * out.h * out.w * c8;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_upsample_nearest<T>, grid_for(total), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, c8, stride, scale));
    return hipGetLastError();
}

template <typename T>
__global__ void k_scale(T *x, int xs, size_t npix, int C, float scale)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * C) return;
    const size_t p = idx / C; T *q = x + p * xs + (idx - p * C);
    Elt<T>::store1(q, scale * Elt<T>::load1(q));
}
hipError_t launch_scale(const TView &x, float scale, hipStream_t s)
{
    if (x.dt == DT_FP8) return hipErrorInvalidValue;
    const size_t npix = (size_t)x.n * x.h * x.w;
    WITH_DT(x.dt, hipLaunchKernelGGL(k_scale<T>, grid_for(npix * x.c), dim3(256), 0, s, (T *)x.ptr, x.stride, npix, x.c, scale));
    return hipGetLastError();
}

template <typename T>
__global__ void k_copy_channels(const T *in, int is, T *out, int os, size_t npix, int C, int Cw)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * Cw) return;
    const size_t p = idx / Cw; const int c = (int)(idx - p * Cw);
    if (c < C) out[p * os + c] = in[p * is + c];
    else Elt<T>::store1(out + p * os + c, 0.f);
}
// `zero_to` > in.c: channels in.c .. zero_to of every output pixel are stored as zeros (the tail of a concatenation's last granule)
hipError_t launch_copy_channels(const TView &in, const TView &out, hipStream_t s, int zero_to)
{
    const int cw = std::max(in.c, zero_to);
    if (in.dt != out.dt || in.c != out.c || in.c < 1 || in.stride < in.c || out.stride < cw) return hipErrorInvalidValue;
    const size_t npix = (size_t)in.n * in.h * in.w;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_copy_channels<T>, grid_for(npix * cw), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, npix, in.c, cw));
    return hipGetLastError();
}

// ---- labels: per map pixel the first arg-max over the channels (the strict > of first_max keeps the lowest index of a tie), 255 where the
//      maximum is below thresh ----
__device__ __forceinline__ uint8_t pixel_label(const float *p, int c, float thresh)
{
    float best = p[0]; int label = 0;
    for (int k = 1; k < c; ++k) first_max(best, label, p[k], k);
    return best < thresh ? (uint8_t)255 : (uint8_t)label;
}
__global__ void k_label_map(const float *map, int stride, size_t npix, int c, float thresh, uint8_t *labels)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) labels[p] = pixel_label(map + p * stride, c, thresh);
}
hipError_t launch_label_map(const float *map, int stride, size_t npix, int c, float thresh, uint8_t *labels, hipStream_t s)
{
    if (c < 1 || c > 255 || stride < c) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_label_map, grid_for(npix), dim3(256), 0, s, map, stride, npix, c, thresh, labels);
    return hipGetLastError();
}

// image blockIdx.y of a ragged batch: every native pixel looks its map pixel up through the fit (map_coord, kernels.h)
__global__ void k_segment_labels(const float *map, int stride, int map_h, int map_w, int c, float thresh, const ImgDesc *descs, const unsigned long long *label_off,
                                 int fit, int net_h, int net_w, uint8_t *labels)
{
    const int b = blockIdx.y;
    const int h = descs[b].h, w = descs[b].w;
    int new_w = net_w, new_h = net_h;
    if (fit == FIT_LETTERBOX) letterbox_dims(net_w, net_h, w, h, &new_w, &new_h);
    const int dx = (net_w - new_w) / 2, dy = (net_h - new_h) / 2;          // DN/image.c:960-981: the fitted image sits centred
    uint8_t *out = labels + label_off[b];
    const float *m = map + (size_t)b * map_h * map_w * stride;
    const size_t total = (size_t)h * w;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / w), x = (int)(p - (size_t)y * w);
        const int my = map_coord(y, h, new_h, dy, net_h, map_h), mx = map_coord(x, w, new_w, dx, net_w, map_w);
        out[p] = pixel_label(m + ((size_t)my * map_w + mx) * stride, c, thresh);
    }
}
hipError_t launch_segment_labels(const float *map, int stride, int map_h, int map_w, int c, float thresh, const ImgDesc *descs, const unsigned long long *label_off,
                                 int n, int fit, int net_h, int net_w, uint8_t *labels, hipStream_t s)
{
    if (c < 1 || c > 255 || stride < c || n < 1 || n > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_segment_labels, dim3(256, (unsigned)n), dim3(256), 0, s, map, stride, map_h, map_w, c, thresh, descs, label_off, fit, net_h, net_w, labels);
    return hipGetLastError();
}

__global__ void k_nhwc_to_chw(const float *in, float *out, int hw, int c, size_t total)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // over the output [n][c][hw]
    if (idx >= total) return;
    const size_t per = (size_t)hw * c, b = idx / per, r = idx - b * per;
    const int ch = (int)(r / hw), q = (int)(r - (size_t)ch * hw);
    out[idx] = in[b * per + (size_t)q * c + ch];
}
hipError_t launch_nhwc_to_chw(const float *in, float *out, int n, int hw, int c, hipStream_t s)
{
    const size_t total = (size_t)n * hw * c;
    hipLaunchKernelGGL(k_nhwc_to_chw, grid_for(total), dim3(256), 0, s, in, out, hw, c, total);
    return hipGetLastError();
}
