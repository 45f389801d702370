// HBM-bound NHWC operators around the conv stack: input conversion / stretch-resize (row P), 2x
// upsample (row U), max-pool (row M), space-to-depth / darknet reorg (row R), residual add and strided
// copies (rows B, Rt when they cannot be fused into a conv epilogue), dtype conversion for introspection.
// One thread moves an 8-channel granule (16 B of bf16, 32 B of fp32) so global accesses are 16-B vectors
// and consecutive lanes touch consecutive addresses along the channel axis.  A tensor of C channels has ceil(C / 8) granules: its pixel
// stride is a multiple of 8, and the channels C .. of the last granule are zeros that every layer stores again (a consumer multiplies
// them by zero filters; a stale Inf or NaN there would not survive that).
#include "kernels.h"
#include "device_common.h"
#include "activations.h"
#include <math.h>
#include <algorithm>

#include "elt.h"

// do `c` channels fit both pixel strides as whole 8-channel granules?
static inline bool granules_ok(int c, int stride_a, int stride_b) { const int c8 = (c + 7) / 8; return c >= 1 && stride_a >= c8 * 8 && stride_b >= c8 * 8; }

// ---- The channel count of the staging kernels below.  NCH = 3: an RGB image, one lane per output pixel, its one granule 3 real + 5 zero channels.
//      NCH = 0: `nch` planes ([net] yolo_input=planes), one lane per output pixel x 8-channel granule; the granule is the SLOW index of the
//      folded grid, so the 64 lanes of a wave read 64 neighbouring pixels of one plane (a planar source: one coalesced run per channel; a packed
//      one: bytes `nch` apart) and each stores its granule as one vector.  The channels nch .. of the last granule are stored as zeros. ----
template <int NCH> struct Planes {
    int c0, nc;          // the lane's channels [c0, c0 + nc)
    __device__ __forceinline__ Planes(int g, int nch) : c0(NCH ? 0 : g * 8), nc(NCH ? NCH : min(8, nch - g * 8)) {}
};

// ---- row P: uint8/float image at network size -> whole granules of activation (RGB: 3 real + 5 zero channels) ---------
template <typename T, int NCH>
__global__ void k_preprocess(const void *img, int fmt, size_t npix, size_t hw, float scale, T *out, int out_stride, float post_mul, float post_add, int nch)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t g = NCH ? 0 : idx / npix, p = NCH ? idx : idx - g * npix;
    if (NCH ? p >= npix : g * 8 >= (size_t)nch) return;
    const Planes<NCH> pl((int)g, nch);
    const size_t N = NCH ? NCH : nch;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (fmt == 0) {
        const uint8_t *s = (const uint8_t *)img + p * N + pl.c0;
#pragma unroll
        for (int k = 0; k < (NCH ? NCH : 8); ++k) if (k < pl.nc) v[k] = (float)s[k] * scale;
    } else if (fmt == 1) {
        const float *s = (const float *)img + p * N + pl.c0;
#pragma unroll
        for (int k = 0; k < (NCH ? NCH : 8); ++k) if (k < pl.nc) v[k] = s[k] * scale;
    } else {                                   // planar float [n][N][hw]: darknet's `image` layout (DN/image.c get_pixel)
        const size_t b = p / hw, q = p - b * hw;
        const float *s = (const float *)img + (b * N + pl.c0) * hw + q;
#pragma unroll
        for (int k = 0; k < (NCH ? NCH : 8); ++k) if (k < pl.nc) v[k] = s[k * hw] * scale;
    }
    // YOLOv1's input normalisation `(x / 255) * 2 - 1` (V1/YOLO_V1_Inference.py:67-71): an affine map of the real channels
    if (post_mul != 1.0f || post_add != 0.0f) {
#pragma unroll
        for (int k = 0; k < (NCH ? NCH : 8); ++k) if (k < pl.nc) v[k] = v[k] * post_mul + post_add;
    }
    Elt<T>::store8(out + p * out_stride + pl.c0, v);
}

hipError_t launch_preprocess(const void *img, int fmt, int n, int hw, float scale, void *out, int out_dt,
                             int out_stride, hipStream_t s, float post_mul, float post_add, int nch)
{
    size_t npix = (size_t)n * hw;
    if (nch < 1 || out_stride < (nch + 7) / 8 * 8) return hipErrorInvalidValue;
    if (nch == 3) WITH_DT(out_dt, hipLaunchKernelGGL((k_preprocess<T, 3>), grid_for(npix), dim3(256), 0, s, img, fmt, npix, (size_t)hw, scale, (T *)out, out_stride, post_mul, post_add, 3));
    else WITH_DT(out_dt, hipLaunchKernelGGL((k_preprocess<T, 0>), grid_for(npix * ((nch + 7) / 8)), dim3(256), 0, s, img, fmt, npix, (size_t)hw, scale, (T *)out, out_stride, post_mul, post_add, nch));
    return hipGetLastError();
}

// ---- per-pixel arithmetic of the image fits, shared by the single-image kernels and the batched k_fit_images.  `at(y, x, c)`
//      returns what the fit reads at a source pixel: the byte as a float for the stretch and cv2 forms, the 0..1 value for the letterbox
//      and the centre crop (a planar float image, or a byte through fit_unit_value).  Restated operation for operation from the reference; this file is
//      compiled with -ffp-contract=off, so every caller rounds the same.  Coordinates and weights are computed once; then the channels
//      [c0, c0 + nc) are interpolated into v[0 .. nc): NC = 3 is the RGB form (c0 = 0, nc = 3 at every call), NC = 8 one granule of an N-plane image. ----

// legacy TF bilinear (no half-pixel offset): src = dst * (in/out); value/255 first (D2T _input_process)
template <int NC, class At>
__device__ __forceinline__ void px_stretch(const At &at, int h, int w, int oh, int ow, int oy, int ox, float post_scale, float post_add, int c0, int nc, float *v)
{
    const float hs = (float)h / (float)oh, ws = (float)w / (float)ow;
    float fy = (float)oy * hs, fx = (float)ox * ws;
    int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    float yl = fy - (float)y0, xl = fx - (float)x0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        if (NC != 3 && k >= nc) break;
        const int c = c0 + k;
        float tl = at(y0, x0, c) / 255.0f;
        float tr = at(y0, x1, c) / 255.0f;
        float bl = at(y1, x0, c) / 255.0f;
        float br = at(y1, x1, c) / 255.0f;
        float top = tl + (tr - tl) * xl;
        float bot = bl + (br - bl) * xl;
        v[k] = top + (bot - top) * yl;
        if (post_scale != 1.0f) v[k] *= post_scale;
        if (post_add != 0.0f) v[k] += post_add;
    }
}

// darknet resize_image (DN/image.c:1347-1393) of an iw x ih image to new_w x new_h, evaluated at ONE pixel (r, c) of the result: horizontal
// pass then vertical pass, scales (in-1)/(out-1), last column / row copied.  Operation order of the two passes is kept:
// part = (1-dx)*a + dx*b, then (1-dy)*p0 (+ dy*p1).  Where the size does not change the scales are 1, dx = dy = 0, and the value is the
// source pixel itself, bit for bit: resize_min's `no resize` branch (DN/image.c:1008) needs no case of its own.
template <int NC, class At>
__device__ __forceinline__ void px_resize(const At &at, int iw, int ih, int new_w, int new_h, int r, int c, int c0, int nc, float *v)
{
    const float w_scale = (float)(iw - 1) / (float)(new_w - 1), h_scale = (float)(ih - 1) / (float)(new_h - 1);
    const float sy = (float)r * h_scale; const int iy = (int)sy; const float dy = sy - (float)iy;
    const bool last_c = c == new_w - 1 || iw == 1, last_r = r == new_h - 1 || ih == 1;
    const float sx = (float)c * w_scale; const int ix = (int)sx; const float dx = sx - (float)ix;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        if (NC != 3 && k >= nc) break;
        const int ch = c0 + k;
        auto part = [&](int row) {
            if (last_c) return at(row, iw - 1, ch);
            return (1 - dx) * at(row, ix, ch) + dx * at(row, ix + 1, ch);
        };
        float val = (1 - dy) * part(iy);
        if (!last_r) val = val + dy * part(iy + 1);
        v[k] = val;
    }
}

// darknet letterbox_image (DN/image.c:960-981) of one output pixel: the aspect-preserving resize_image embedded at the centre of a
// 0.5-filled canvas (the fill belongs to the real channels: a granule's padding stays zero).
template <int NC, class At>
__device__ __forceinline__ void px_letterbox(const At &at, int iw, int ih, int new_w, int new_h, int off_x, int off_y, int oy, int ox, int c0, int nc, float *v)
{
    const int r = oy - off_y, c = ox - off_x;
#pragma unroll
    for (int k = 0; k < NC; ++k) if (NC == 3 || k < nc) v[k] = 0.5f;
    if ((unsigned)r < (unsigned)new_h && (unsigned)c < (unsigned)new_w) px_resize<NC>(at, iw, ih, new_w, new_h, r, c, c0, nc, v);
}

// darknet's classifier validation fit (DN/examples/classifier.c:635-636) of one output pixel: resize_min(im, net_w) -- the shorter side
// becomes net_w, whatever net_h is -- then crop_image(resized, (rw - net_w) / 2, (rh - net_h) / 2, net_w, net_h) (DN/image.c:857-875).  The
// offsets truncate toward zero and are negative where the resized image is smaller than the network (a non-square one); the coordinates
// are CLAMPED to the resized image, so its edge is replicated: there is no fill value.
template <int NC, class At>
__device__ __forceinline__ void px_center_crop(const At &at, int iw, int ih, int net_w, int net_h, int oy, int ox, int c0, int nc, float *v)
{
    int rw, rh;
    resize_min_dims(net_w, iw, ih, &rw, &rh);
    const int r = min(max(oy + (rh - net_h) / 2, 0), rh - 1), c = min(max(ox + (rw - net_w) / 2, 0), rw - 1);
    px_resize<NC>(at, iw, ih, rw, rh, r, c, c0, nc, v);
}

// One pixel of one of darknet's ten validation views (DN/examples/classifier.c:268-283, `classifier valid10`): the image resized to R = (net_w + shift) x
// (net_h + shift) -- load_image_color's resize_image, the image itself where it has that size --, then crop_image(R, dx, dy, net_w, net_h) with dx, dy in
// {-shift, 0, shift}: the coordinates are CLAMPED to R (the -shift views replicate its edge; the (0, 0) view is the top-left window, not the centre), and
// the views 5..9 crop flip_image(R): column c of the mirrored image is column rw - 1 - c of R.  No R is ever stored: px_resize at that coordinate.
template <int NC, class At>
__device__ __forceinline__ void px_ten_crop(const At &at, int iw, int ih, int net_w, int net_h, int shift, int dy, int dx, int flip, int oy, int ox, int c0, int nc, float *v)
{
    const int rw = net_w + shift, rh = net_h + shift;
    const int r = min(max(oy + dy, 0), rh - 1), c = min(max(ox + dx, 0), rw - 1);
    px_resize<NC>(at, iw, ih, rw, rh, r, flip ? rw - 1 - c : c, c0, nc, v);
}

// `cv2.resize(image_float32, (ow, oh))` as V2/utils.py:13-27 calls it (INTER_LINEAR on a float32 image, after BGR -> RGB) followed by the
// reference's `/ 225.0` -- restated from OpenCV's published resize (imgproc/resize.cpp, the CV_32F linear path): half-pixel centres,
//   fx = (float)((dx + 0.5) * (double)(src_w / dst_w as 1 / (dst_w / src_w)) - 0.5); sx = floor(fx); fx -= sx;
//   sx < 0 -> (sx, fx) = (0, 0);  sx >= src_w - 1 -> (sx, fx) = (src_w - 1, 0);     likewise in y,
// a horizontal pass S[sx] * (1 - fx) + S[sx + 1] * fx on both rows, then the vertical one R0 * (1 - fy) + R1 * fy (separately rounded
// float operations).  cv2 is absent here: parity unpinned, oracle.resize_cv2_linear is the same closed form.  swap_rb: output channel c
// reads input channel 2 - c (cv2.cvtColor(..., COLOR_BGR2RGB)).
template <class At>
__device__ __forceinline__ void px_cv2(const At &at, int h, int w, int oh, int ow, int dy, int dx, int swap_rb, float divisor, float *v)
{
    const double scale_x = 1.0 / ((double)ow / (double)w), scale_y = 1.0 / ((double)oh / (double)h);
    float fx = (float)(((double)dx + 0.5) * scale_x - 0.5), fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
    int sx = (int)floorf(fx), sy = (int)floorf(fy);
    fx -= (float)sx; fy -= (float)sy;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= w - 1) { sx = w - 1; fx = 0.f; }
    if (sy < 0) { sy = 0; fy = 0.f; }
    if (sy >= h - 1) { sy = h - 1; fy = 0.f; }
    const int sx1 = min(sx + 1, w - 1), sy1 = min(sy + 1, h - 1);
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int ci = swap_rb ? 2 - c : c;
        const float p00 = at(sy, sx, ci), p01 = at(sy, sx1, ci);
        const float p10 = at(sy1, sx, ci), p11 = at(sy1, sx1, ci);
        const float r0 = p00 * a0 + p01 * a1, r1 = p10 * a0 + p11 * a1;
        v[c] = (r0 * b0 + r1 * b1) / divisor;
    }
}

// source readers of the single-image kernels: a uint8 HWC image of `px` channels, a planar float [C][h][w] image
struct AtU8 {
    const uint8_t *img; int w, px;
    __device__ __forceinline__ float operator()(int y, int x, int c) const { return (float)img[((size_t)y * w + x) * px + c]; }
};
struct AtPlanar {
    const float *img; int w, h;
    __device__ __forceinline__ float operator()(int y, int x, int k) const { return img[(size_t)k * w * h + (size_t)y * w + x]; }
};

template <typename T, int NCH>
__global__ void k_resize_u8(const uint8_t *img, int h, int w, int oh, int ow, T *out, int out_stride, int out_c, float post_scale, float post_add, int nch)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = NCH ? 0 : idx / (oh * ow), p = NCH ? idx : idx - g * (oh * ow);
    if (NCH ? p >= oh * ow : g * 8 >= nch) return;
    const Planes<NCH> pl(g, nch);
    int oy = p / ow, ox = p - oy * ow;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    px_stretch<NCH ? NCH : 8>(AtU8{img, w, NCH ? NCH : nch}, h, w, oh, ow, oy, ox, post_scale, post_add, pl.c0, pl.nc, v);
    if (out_c >= 8) Elt<T>::store8(out + (size_t)p * out_stride + pl.c0, v);
    else
        for (int c = 0; c < out_c; ++c) Elt<T>::store1(out + (size_t)p * out_stride + c, v[c]);
}

// nch != 3: whole granules are stored (out_c >= nch, out_stride >= roundup(nch, 8))
hipError_t launch_resize_u8(const uint8_t *img, int h, int w, int out_h, int out_w, void *out, int out_dt, int out_stride,
                            int out_c, hipStream_t s, float post_scale, float post_add, int nch)
{
    size_t np = (size_t)out_h * out_w;
    if (nch == 3) { WITH_DT(out_dt, hipLaunchKernelGGL((k_resize_u8<T, 3>), grid_for(np), dim3(256), 0, s, img, h, w, out_h, out_w, (T *)out, out_stride, out_c, post_scale, post_add, 3)); return hipGetLastError(); }
    const int c8 = (nch + 7) / 8;
    if (nch < 1 || out_c < 8 || out_stride < c8 * 8 || np * c8 > 0x7fffffffull) return hipErrorInvalidValue;
    WITH_DT(out_dt, hipLaunchKernelGGL((k_resize_u8<T, 0>), grid_for(np * c8), dim3(256), 0, s, img, h, w, out_h, out_w, (T *)out, out_stride, out_c, post_scale, post_add, nch));
    return hipGetLastError();
}

// cv2.resize of one uint8 image to fp32 [oh][ow][3] (px_cv2 above)
__global__ void k_resize_cv2_u8(const uint8_t *img, int h, int w, int oh, int ow, int swap_rb, float divisor, float *out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= oh * ow) return;
    const int dy = p / ow, dx = p - dy * ow;
    float v[3];
    px_cv2(AtU8{img, w, 3}, h, w, oh, ow, dy, dx, swap_rb, divisor, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(size_t)p * 3 + c] = v[c];
}
hipError_t launch_resize_cv2_u8(const uint8_t *img, int h, int w, int oh, int ow, int swap_rb, float divisor, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_resize_cv2_u8, grid_for((size_t)oh * ow), dim3(256), 0, s, img, h, w, oh, ow, swap_rb, divisor, out);
    return hipGetLastError();
}

// ---- row U: 2x upsample.  bilinear = closed form of pad(SYMMETRIC 1) -> legacy resize_bilinear -> crop,
//      evaluated with TF's lerp order (x then y, a + (b-a)*t, t in {0, .5}); else nearest (darknet). ----
template <typename T>
__global__ void k_upsample2x(const T *in, int is, T *out, int os, int n, int h, int w, int c8, int bilinear)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)n * 2 * h * 2 * w * c8;
    if (idx >= total) return;
    int g = (int)(idx % c8); size_t p = idx / c8;
    int ox = (int)(p % (2 * w)); p /= (2 * w);
    int oy = (int)(p % (2 * h)); int b = (int)(p / (2 * h));
    int iy = oy >> 1, ix = ox >> 1;
    const T *base = in + (size_t)b * h * w * is + g * 8;
    float r[8];
    if (!bilinear) {
        Elt<T>::load8(base + ((size_t)iy * w + ix) * is, r);
    } else {
        int iy1 = min(iy + 1, h - 1), ix1 = min(ix + 1, w - 1);
        float xl = (ox & 1) ? 0.5f : 0.f, yl = (oy & 1) ? 0.5f : 0.f;
        float tl[8], tr[8], bl[8], br[8];
        Elt<T>::load8(base + ((size_t)iy * w + ix) * is, tl);
        Elt<T>::load8(base + ((size_t)iy * w + ix1) * is, tr);
        Elt<T>::load8(base + ((size_t)iy1 * w + ix) * is, bl);
        Elt<T>::load8(base + ((size_t)iy1 * w + ix1) * is, br);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float top = tl[i] + (tr[i] - tl[i]) * xl;
            float bot = bl[i] + (br[i] - bl[i]) * xl;
            r[i] = top + (bot - top) * yl;
        }
    }
    Elt<T>::store8(out + (((size_t)b * 2 * h + oy) * 2 * w + ox) * os + g * 8, r);
}

hipError_t launch_upsample2x(const TView &in, const TView &out, int bilinear, hipStream_t s)
{
    if (in.dt != out.dt || !granules_ok(in.c, in.stride, out.stride)) return hipErrorInvalidValue;
    const int c8 = (in.c + 7) / 8;
    size_t total = (size_t)in.n * 4 * in.h * in.w * c8;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_upsample2x<T>, grid_for(total), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, c8, bilinear));
    return hipGetLastError();
}

// ---- row M: max-pool, window origin -pad, out-of-range = -inf (DN/maxpool_layer.c:79-111 == TF); the lanes at and beyond channel `c` of
//      the last granule are stored as zeros whatever the window held ----
template <typename T>
__global__ void k_maxpool(const T *in, int is, T *out, int os, int n, int h, int w, int ho, int wo, int c8, int c,
                          int size, int stride, int pad)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)n * ho * wo * c8;
    if (idx >= total) return;
    int g = (int)(idx % c8); size_t p = idx / c8;
    int ox = (int)(p % wo); p /= wo;
    int oy = (int)(p % ho); int b = (int)(p / ho);
    float m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = -INFINITY;
    for (int dy = 0; dy < size; ++dy)
        for (int dx = 0; dx < size; ++dx) {
            int iy = oy * stride + dy - pad, ix = ox * stride + dx - pad;
            if ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) {
                float v[8];
                Elt<T>::load8(in + (((size_t)b * h + iy) * w + ix) * is + g * 8, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) m[i] = v[i] > m[i] ? v[i] : m[i];
            }
        }
    if (g * 8 + 8 > c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) if (g * 8 + i >= c) m[i] = 0.f;
    }
    Elt<T>::store8(out + (((size_t)b * ho + oy) * wo + ox) * os + g * 8, m);
}

hipError_t launch_maxpool(const TView &in, const TView &out, int size, int stride, int pad, hipStream_t s)
{
    if (in.dt != out.dt || !granules_ok(in.c, in.stride, out.stride) || size < 1 || stride < 1 || pad < 0) return hipErrorInvalidValue;
    const int c8 = (in.c + 7) / 8;
    size_t total = (size_t)out.n * out.h * out.w * c8;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_maxpool<T>, grid_for(total), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, out.h, out.w, c8, in.c, size, stride, pad));
    return hipGetLastError();
}

// ---- row R: tf.space_to_depth (granule copy) or darknet reorg_cpu(forward=0) (element scramble) ----
template <typename T>
__global__ void k_space_to_depth(const T *in, int is, T *out, int os, int n, int h, int w, int c8, int st)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)n * h * w * c8;
    if (idx >= total) return;
    int g = (int)(idx % c8); size_t p = idx / c8;
    int ix = (int)(p % w); p /= w;
    int iy = (int)(p % h); int b = (int)(p / h);
    float v[8];
    Elt<T>::load8(in + (((size_t)b * h + iy) * w + ix) * is + g * 8, v);
    int oy = iy / st, dy = iy - oy * st, ox = ix / st, dx = ix - ox * st;
    int oc = (dy * st + dx) * (c8 * 8) + g * 8;
    Elt<T>::store8(out + (((size_t)b * (h / st) + oy) * (w / st) + ox) * os + oc, v);
}

// ... for a channel count that is no multiple of 8 (block (dy, dx) begins at channel (dy * st + dx) * c, not at a granule): one output
// element per lane; the channels c * st * st .. cw of an output pixel are stored as zeros
template <typename T>
__global__ void k_space_to_depth_elems(const T *in, int is, T *out, int os, int n, int h, int w, int c, int st, int cw)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ho = h / st, wo = w / st;
    if (idx >= (size_t)n * ho * wo * cw) return;
    const int co = (int)(idx % cw); size_t p = idx / cw;
    const int ox = (int)(p % wo); p /= wo;
    const int oy = (int)(p % ho), b = (int)(p / ho);
    float v = 0.f;
    if (co < c * st * st) {
        const int blk = co / c, ch = co - blk * c, dy = blk / st, dx = blk - dy * st;
        v = Elt<T>::load1(in + (((size_t)b * h + oy * st + dy) * w + ox * st + dx) * is + ch);
    }
    Elt<T>::store1(out + (((size_t)b * ho + oy) * wo + ox) * os + co, v);
}

// Darknet: with x,out as NCHW flat buffers of the *input* geometry (w,h,c): out[in_index] = x[out_index]
// (DN/blas.c:9-30, forward=0), the result then reinterpreted as [c*s*s, h/s, w/s].  `cw` >= c*s*s: the channels of an output pixel that
// are stored; those past c*s*s (t >= h*w*c below) as zeros.
template <typename T>
__global__ void k_reorg_darknet(const T *in, int is, T *out, int os, int n, int h, int w, int c, int st, int cw)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t per = (size_t)(h / st) * (w / st) * cw;
    if (idx >= per * n) return;
    int b = (int)(idx / per); int t = (int)(idx - (size_t)b * per);      // t = in_index
    if (t >= h * w * c) {
        const int wz = w / st, hz = h / st;
        Elt<T>::store1(out + (((size_t)b * hz + (t / wz) % hz) * wz + t % wz) * os + t / (wz * hz), 0.f);
        return;
    }
    int i = t % w, j = (t / w) % h, k = t / (w * h);
    int out_c = c / (st * st);
    int c2 = k % out_c, off = k / out_c;
    int w2 = i * st + off % st, h2 = j * st + off / st;
    int src = w2 + w * st * (h2 + h * st * c2);                          // flat NCHW index into x viewed as [out_c, h*st, w*st]
    // x is the input tensor [c, h, w] NCHW flat: decode src as (cs, ys, xs) of that geometry
    int xs = src % w, ys = (src / w) % h, cs = src / (w * h);
    float v = Elt<T>::load1(in + (((size_t)b * h + ys) * w + xs) * is + cs);
    // destination flat index t of a buffer reinterpreted as [c*st*st, h/st, w/st]
    int wo = w / st, ho = h / st;
    int xo = t % wo, yo = (t / wo) % ho, co = t / (wo * ho);
    Elt<T>::store1(out + (((size_t)b * ho + yo) * wo + xo) * os + co, v);
}

hipError_t launch_reorg(const TView &in, const TView &out, int stride, int darknet, hipStream_t s)
{
    if (in.dt != out.dt || stride < 1 || in.c < 1 || in.h % stride || in.w % stride || in.stride < in.c) return hipErrorInvalidValue;
    const int co = in.c * stride * stride, cw = std::min(out.stride, (co + 7) / 8 * 8);      // the stored channels of an output pixel: whole granules
    if (out.stride < co || (size_t)in.h * in.w * in.c + (size_t)in.h * in.w * 8 > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t elems = (size_t)in.n * (in.h / stride) * (in.w / stride) * cw;
    if (!darknet && in.c % 8 == 0) {
        size_t total = (size_t)in.n * in.h * in.w * (in.c / 8);
        WITH_DT(in.dt, hipLaunchKernelGGL(k_space_to_depth<T>, grid_for(total), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, in.c / 8, stride));
    } else if (!darknet) {
        WITH_DT(in.dt, hipLaunchKernelGGL(k_space_to_depth_elems<T>, grid_for(elems), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, in.c, stride, cw));
    } else {
        if (in.c < stride * stride) return hipErrorInvalidValue;      // reorg_cpu divides by c / (stride * stride)
        WITH_DT(in.dt, hipLaunchKernelGGL(k_reorg_darknet<T>, grid_for(elems), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, in.n, in.h, in.w, in.c, stride, cw));
    }
    return hipGetLastError();
}

// ---- rows B / Rt fallbacks: residual add and strided copy --------------------------------------
template <typename T>
__global__ void k_add(const T *a, int as, const T *b, int bs, T *o, int os, size_t npix, int c8, float sa, float sb, float so)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    size_t p = idx / c8; int g = (int)(idx - p * c8);
    float x[8], y[8];
    Elt<T>::load8(a + p * as + g * 8, x);
    Elt<T>::load8(b + p * bs + g * 8, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = (x[i] * sa + y[i] * sb) * so;       // scales are exactly 1 unless fp8
    Elt<T>::store8(o + p * os + g * 8, x);
}
hipError_t launch_add(const TView &a, const TView &b, const TView &out, hipStream_t s, float sa, float sb, float so)
{
    if (a.dt != b.dt || a.dt != out.dt || !granules_ok(a.c, a.stride, b.stride) || !granules_ok(a.c, out.stride, out.stride)) return hipErrorInvalidValue;
    size_t npix = (size_t)a.n * a.h * a.w; int c8 = (a.c + 7) / 8;
    WITH_DT(a.dt, hipLaunchKernelGGL(k_add<T>, grid_for(npix * c8), dim3(256), 0, s, (const T *)a.ptr, a.stride, (const T *)b.ptr, b.stride, (T *)out.ptr, out.stride, npix, c8, sa, sb, so));
    return hipGetLastError();
}

template <typename T>
__global__ void k_copy(const T *a, int as, T *o, int os, size_t npix, int c8)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    size_t p = idx / c8; int g = (int)(idx - p * c8);
    float x[8];
    Elt<T>::load8(a + p * as + g * 8, x);
    Elt<T>::store8(o + p * os + g * 8, x);
}
hipError_t launch_copy(const TView &in, const TView &out, hipStream_t s)
{
    if (in.dt != out.dt || !granules_ok(in.c, in.stride, out.stride)) return hipErrorInvalidValue;
    size_t npix = (size_t)in.n * in.h * in.w; int c8 = (in.c + 7) / 8;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_copy<T>, grid_for(npix * c8), dim3(256), 0, s, (const T *)in.ptr, in.stride, (T *)out.ptr, out.stride, npix, c8));
    return hipGetLastError();
}

// ---- dtype conversion between dense fp32 NHWC host-staging buffers and device views -------------
template <typename T>
__global__ void k_to_f32(const T *in, int is, float *out, size_t npix, int c, float scale)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c) return;
    size_t p = idx / c; int ch = (int)(idx - p * c);
    out[idx] = Elt<T>::load1(in + p * is + ch) * scale;
}
hipError_t launch_to_f32(const TView &in, float *out, hipStream_t s, float scale)
{
    size_t npix = (size_t)in.n * in.h * in.w;
    WITH_DT(in.dt, hipLaunchKernelGGL(k_to_f32<T>, grid_for(npix * in.c), dim3(256), 0, s, (const T *)in.ptr, in.stride, out, npix, in.c, scale));
    return hipGetLastError();
}

template <typename T>
__global__ void k_from_f32(const float *in, T *out, int os, size_t npix, int c, float scale)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c) return;
    size_t p = idx / c; int ch = (int)(idx - p * c);
    Elt<T>::store1(out + p * os + ch, in[idx] * scale);
}
hipError_t launch_from_f32(const float *in, const TView &out, hipStream_t s, float scale)
{
    size_t npix = (size_t)out.n * out.h * out.w;
    WITH_DT(out.dt, hipLaunchKernelGGL(k_from_f32<T>, grid_for(npix * out.c), dim3(256), 0, s, in, (T *)out.ptr, out.stride, npix, out.c, scale));
    return hipGetLastError();
}

// ---- split fp16 storage (YOLO_FP16X2): a value v is the pair hi = f16(v), lo = f16(v - hi) -- 22 significant bits out of two 11-bit
//      halves.  A layer output is stored INTERLEAVED (round 6): per 32-channel group 32 hi then 32 lo, [pixel][2 * Cp], Cp = channels rounded
//      up to 32 -- a 128-byte run of a pixel is one K-step row [hi | lo] of the conv that reads it, which forms W_hi x_hi + W_lo x_hi +
//      W_hi x_lo from it (conv_igemm_kernel.h, PAIRK; what is dropped is W_lo x_lo, 2^-22 of the product).  The network input keeps rounds
//      4-5's three blocks hi | lo | hi of its 8 padded channels (PAIR_B3), read by an ordinary fp16 K loop against W_hi | W_hi | W_lo.
//      These are the memory-bound pieces around the convs. ----
__device__ __forceinline__ void split8(const float *v, uint4 &H, uint4 &L)
{
    typedef Elt<f16_t> E;
    H = uint4{E::pk(v[0], v[1]), E::pk(v[2], v[3]), E::pk(v[4], v[5]), E::pk(v[6], v[7])};
    const uint32_t w[4] = {H.x, H.y, H.z, H.w};
    float lo[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const E::h2 h = __builtin_bit_cast(E::h2, w[i]); lo[2 * i] = v[2 * i] - (float)h[0]; lo[2 * i + 1] = v[2 * i + 1] - (float)h[1]; }
    L = uint4{E::pk(lo[0], lo[1]), E::pk(lo[2], lo[3]), E::pk(lo[4], lo[5]), E::pk(lo[6], lo[7])};
}
// element offset of the hi piece of channels [g * 8, g * 8 + 8) inside a pixel, and the distance to its lo piece
__device__ __forceinline__ int pair_hi_off(int g, int Cp, int layout) { const int c = g * 8; return layout == PAIR_B3 ? c : (c >> 5) * 64 + (c & 31); }
__device__ __forceinline__ int pair_lo_dist(int Cp, int layout) { return layout == PAIR_B3 ? Cp : 32; }
__device__ __forceinline__ void join8(const f16_t *p, int lo_dist, float *v)
{
    float h[8], l[8];
    Elt<f16_t>::load8(p, h); Elt<f16_t>::load8(p + lo_dist, l);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h[i] + l[i];
}
__device__ __forceinline__ void put_split8(f16_t *p, int Cp, int layout, const float *v)
{
    uint4 H, L; split8(v, H, L);
    *(uint4 *)p = H; *(uint4 *)(p + pair_lo_dist(Cp, layout)) = L;
    if (layout == PAIR_B3) *(uint4 *)(p + 2 * Cp) = H;
}
__global__ void k_split_from_f32(const float *in, int is, f16_t *out, int os, int Cp, size_t npix, int layout)
{
    const int c8 = Cp / 8;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    size_t p = idx / c8; int g = (int)(idx - p * c8);
    float v[8]; Elt<float>::load8(in + p * is + g * 8, v);
    put_split8(out + p * os + pair_hi_off(g, Cp, layout), Cp, layout, v);
}
__global__ void k_split_to_f32(const f16_t *in, int is, int Cp, float *out, int os, size_t npix, int layout)
{
    const int c8 = Cp / 8;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    size_t p = idx / c8; int g = (int)(idx - p * c8);
    float v[8]; join8(in + p * is + pair_hi_off(g, Cp, layout), pair_lo_dist(Cp, layout), v);
    Elt<float>::store8(out + p * os + g * 8, v);
}
// shortcut on split tensors: (a_hi + a_lo) + (b_hi + b_lo), split again (each parenthesis is exact in fp32 when the pair came from split8)
__global__ void k_add_split(const f16_t *a, int as, const f16_t *b, int bs, f16_t *o, int os, int Cp, size_t npix)
{
    const int c8 = Cp / 8;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    size_t p = idx / c8; int g = (int)(idx - p * c8);
    const int ho = pair_hi_off(g, Cp, PAIR_ILV);
    float x[8], y[8];
    join8(a + p * as + ho, 32, x); join8(b + p * bs + ho, 32, y);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = x[i] + y[i];
    put_split8(o + p * os + ho, Cp, PAIR_ILV, x);
}
// 2x upsample of an interleaved pair tensor in ONE launch: join (hi + lo), the fp32 kernel's arithmetic (k_upsample2x: TF's lerp order, or
// nearest), split -- bit-identical to the join / fp32 upsample / split sequence it replaces (three launches through fp32 staging)
__global__ void k_upsample2x_pair(const f16_t *in, int is, f16_t *out, int os, int n, int h, int w, int Cp, int bilinear)
{
    const int c8 = Cp / 8;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)n * 2 * h * 2 * w * c8;
    if (idx >= total) return;
    const int g = (int)(idx % c8); size_t p = idx / c8;
    const int ox = (int)(p % (2 * w)); p /= (2 * w);
    const int oy = (int)(p % (2 * h)); const int b = (int)(p / (2 * h));
    const int iy = oy >> 1, ix = ox >> 1, ho = pair_hi_off(g, Cp, PAIR_ILV);
    const f16_t *base = in + (size_t)b * h * w * is + ho;
    f16_t *o = out + (((size_t)b * 2 * h + oy) * 2 * w + ox) * os + ho;
    if (!bilinear) {          // nearest: join and split again, as the fp32 sequence does (split(join(hi, lo)) may choose another pair for the same value at a tie)
        float v[8]; join8(base + ((size_t)iy * w + ix) * is, 32, v);
        put_split8(o, Cp, PAIR_ILV, v);
        return;
    }
    const int iy1 = min(iy + 1, h - 1), ix1 = min(ix + 1, w - 1);
    const float xl = (ox & 1) ? 0.5f : 0.f, yl = (oy & 1) ? 0.5f : 0.f;
    float tl[8], tr[8], bl[8], br[8], r[8];
    join8(base + ((size_t)iy * w + ix) * is, 32, tl); join8(base + ((size_t)iy * w + ix1) * is, 32, tr);
    join8(base + ((size_t)iy1 * w + ix) * is, 32, bl); join8(base + ((size_t)iy1 * w + ix1) * is, 32, br);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float top = tl[i] + (tr[i] - tl[i]) * xl;
        const float bot = bl[i] + (br[i] - bl[i]) * xl;
        r[i] = top + (bot - top) * yl;
    }
    put_split8(o, Cp, PAIR_ILV, r);
}
hipError_t launch_upsample2x_pair(const TView &in, const TView &out, int bilinear, hipStream_t s)
{
    const int Cp = (in.c + 31) / 32 * 32;
    if (in.dt != DT_F16 || out.dt != DT_F16 || in.stride < 2 * Cp || out.stride < 2 * Cp) return hipErrorInvalidValue;
    const size_t total = (size_t)in.n * 4 * in.h * in.w * (Cp / 8);
    hipLaunchKernelGGL(k_upsample2x_pair, grid_for(total), dim3(256), 0, s, (const f16_t *)in.ptr, in.stride, (f16_t *)out.ptr, out.stride, in.n, in.h, in.w, Cp, bilinear);
    return hipGetLastError();
}
hipError_t launch_split_from_f32(const float *in, int in_stride, void *out, int out_stride, int Cp, size_t npix, hipStream_t s, int layout)
{
    hipLaunchKernelGGL(k_split_from_f32, grid_for(npix * (Cp / 8)), dim3(256), 0, s, in, in_stride, (f16_t *)out, out_stride, Cp, npix, layout);
    return hipGetLastError();
}
hipError_t launch_split_to_f32(const void *in, int in_stride, int Cp, float *out, int out_stride, size_t npix, hipStream_t s, int layout)
{
    hipLaunchKernelGGL(k_split_to_f32, grid_for(npix * (Cp / 8)), dim3(256), 0, s, (const f16_t *)in, in_stride, Cp, out, out_stride, npix, layout);
    return hipGetLastError();
}
hipError_t launch_add_split(const void *a, int a_stride, const void *b, int b_stride, void *out, int out_stride, int Cp, size_t npix, hipStream_t s)
{
    hipLaunchKernelGGL(k_add_split, grid_for(npix * (Cp / 8)), dim3(256), 0, s, (const f16_t *)a, a_stride, (const f16_t *)b, b_stride, (f16_t *)out, out_stride, Cp, npix);
    return hipGetLastError();
}

// ---- activations and the general [shortcut] (DN/activations.h, DN/blas.c:68-92 shortcut_cpu) ----
// k_activate: x = act(x) in place on the C real channels of a view (channels C .. of the last granule keep their zeros); one 16-byte granule
// per lane: 8 channels of a 16-bit tensor, 4 of an fp32 one (an fp32 head's pixel stride is a multiple of 4 only).  G = channels per granule.
template <typename T, int G>
__global__ void k_activate(T *x, int xs, size_t npix, int C, int cg, int act)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * cg) return;
    const size_t p = idx / cg; const int g = (int)(idx - p * cg);
    T *q = x + p * xs + g * G;
    if constexpr (G == 4) {
        float4 v = *(const float4 *)q;
        float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) if (g * 4 + i < C) r[i] = act_apply(r[i], act);
        *(float4 *)q = float4{r[0], r[1], r[2], r[3]};
    } else {
        float r[8];
        Elt<T>::load8(q, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) if (g * 8 + i < C) r[i] = act_apply(r[i], act);
        Elt<T>::store8(q, r);
    }
}
// ... on an interleaved split-fp16 pair tensor: join, activate, split again
__global__ void k_activate_pair(f16_t *x, int xs, size_t npix, int C, int Cp, int act)
{
    const int c8 = Cp / 8;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * c8) return;
    const size_t p = idx / c8; const int g = (int)(idx - p * c8);
    f16_t *q = x + p * xs + pair_hi_off(g, Cp, PAIR_ILV);
    float r[8]; join8(q, 32, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) if (g * 8 + i < C) r[i] = act_apply(r[i], act);
    put_split8(q, Cp, PAIR_ILV, r);
}
hipError_t launch_activate(const TView &x, bool pair, int act, hipStream_t s)
{
    if (act < 0 || act >= ACT_COUNT || x.dt == DT_FP8) return hipErrorInvalidValue;
    if (act == ACT_LINEAR) return hipSuccess;
    const size_t npix = (size_t)x.n * x.h * x.w;
    if (pair) {
        const int Cp = (x.c + 31) / 32 * 32;
        if (x.dt != DT_F16 || x.stride < 2 * Cp) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_activate_pair, grid_for(npix * (Cp / 8)), dim3(256), 0, s, (f16_t *)x.ptr, x.stride, npix, x.c, Cp, act);
    } else if (x.dt == DT_F32) {
        const int cg = (x.c + 3) / 4;
        if (x.stride < cg * 4 || x.stride % 4) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_activate<float, 4>), grid_for(npix * cg), dim3(256), 0, s, (float *)x.ptr, x.stride, npix, x.c, cg, act);
    } else {
        const int cg = (x.c + 7) / 8;
        if (x.stride < cg * 8 || x.stride % 8) return hipErrorInvalidValue;
        if (x.dt == DT_F16) hipLaunchKernelGGL((k_activate<f16_t, 8>), grid_for(npix * cg), dim3(256), 0, s, (f16_t *)x.ptr, x.stride, npix, x.c, cg, act);
        else hipLaunchKernelGGL((k_activate<bf16_t, 8>), grid_for(npix * cg), dim3(256), 0, s, (bf16_t *)x.ptr, x.stride, npix, x.c, cg, act);
    }
    return hipGetLastError();
}

// The geometry of shortcut_cpu, restated literally: (w1, h1, c1) the `from` tensor, (w2, h2, c2) the layer's input = output.
__host__ __device__ inline ShortcutGeom shortcut_geom_of(int w1, int h1, int c1, int w2, int h2, int c2)
{
    ShortcutGeom g;
    g.stride = w1 / w2; g.sample = w2 / w1;
    g.ok = g.stride == h1 / h2 && g.sample == h2 / h1;
    if (g.stride < 1) g.stride = 1;
    if (g.sample < 1) g.sample = 1;
    g.minw = w1 < w2 ? w1 : w2; g.minh = h1 < h2 ? h1 : h2; g.minc = c1 < c2 ? c1 : c2;
    return g;
}
ShortcutGeom shortcut_geom(int w1, int h1, int c1, int w2, int h2, int c2) { return shortcut_geom_of(w1, h1, c1, w2, h2, c2); }

// k_shortcut: out = act(a + gather(b)) in one launch, rounded to the storage type once.  a, out: [n, h2, w2, c2]; b (`from`): [n, h1, w1, c1].
// Output position (y, x), channel k receives b[(y / sample) * stride, (x / sample) * stride, k] when k < minc, y and x are multiples of
// `sample` and y / sample < minh, x / sample < minw -- shortcut_cpu's loop read from the output's side; everywhere else the value passes
// through without an add (a + 0 would turn a -0 into +0).  One 8-channel granule per lane; the lanes at and beyond minc of the granule that
// straddles it are masked.  PAIR: interleaved split-fp16 pairs (c1, c2 multiples of 32, so no granule straddles minc).
template <typename T, bool PAIR>
__global__ void k_shortcut(const T *a, int as, const T *b, int bs, T *o, int os, int n, int h2, int w2, int c2, int h1, int w1, ShortcutGeom sg, int act)
{
    const int c8 = PAIR ? ((c2 + 31) / 32 * 32) / 8 : (c2 + 7) / 8;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * h2 * w2 * c8) return;
    const int g = (int)(idx % c8); size_t p = idx / c8;
    const int x = (int)(p % w2); const size_t row = p / w2;
    const int y = (int)(row % h2), img = (int)(row / h2);
    const int off = PAIR ? pair_hi_off(g, c8 * 8, PAIR_ILV) : g * 8;
    float v[8];
    if constexpr (PAIR) join8((const f16_t *)a + p * as + off, 32, v); else Elt<T>::load8(a + p * as + off, v);
    const int j = y / sg.sample, i = x / sg.sample;
    if (g * 8 < sg.minc && j * sg.sample == y && i * sg.sample == x && j < sg.minh && i < sg.minw) {
        const size_t q = ((size_t)img * h1 + (size_t)j * sg.stride) * w1 + (size_t)i * sg.stride;
        float u[8];
        if constexpr (PAIR) join8((const f16_t *)b + q * bs + off, 32, u); else Elt<T>::load8(b + q * bs + off, u);
#pragma unroll
        for (int k = 0; k < 8; ++k) if (g * 8 + k < sg.minc) v[k] = v[k] + u[k];
    }
    if (act != ACT_LINEAR) {
#pragma unroll
        for (int k = 0; k < 8; ++k) if (g * 8 + k < c2) v[k] = act_apply(v[k], act);
    }
    if constexpr (PAIR) put_split8((f16_t *)o + p * os + off, c8 * 8, PAIR_ILV, v); else Elt<T>::store8(o + p * os + off, v);
}
hipError_t launch_shortcut(const TView &a, const TView &b, const TView &out, bool pair, int act, hipStream_t s)
{
    const ShortcutGeom sg = shortcut_geom_of(b.w, b.h, b.c, a.w, a.h, a.c);
    if (!sg.ok || act < 0 || act >= ACT_COUNT || a.dt != b.dt || a.dt != out.dt || a.dt == DT_FP8 || a.n != b.n || out.h != a.h || out.w != a.w || out.c != a.c) return hipErrorInvalidValue;
    if (pair) {
        const int cp2 = (a.c + 31) / 32 * 32;
        if (a.dt != DT_F16 || a.c % 32 || b.c % 32 || a.stride < 2 * cp2 || out.stride < 2 * cp2 || b.stride < 2 * b.c) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_shortcut<f16_t, true>), grid_for((size_t)a.n * a.h * a.w * (cp2 / 8)), dim3(256), 0, s, (const f16_t *)a.ptr, a.stride, (const f16_t *)b.ptr, b.stride,
                           (f16_t *)out.ptr, out.stride, a.n, a.h, a.w, a.c, b.h, b.w, sg, act);
        return hipGetLastError();
    }
    const int c8 = (a.c + 7) / 8;
    if (a.stride < c8 * 8 || out.stride < c8 * 8 || b.stride < (b.c + 7) / 8 * 8) return hipErrorInvalidValue;      // whole granules are read and written
    WITH_DT(a.dt, hipLaunchKernelGGL((k_shortcut<T, false>), grid_for((size_t)a.n * a.h * a.w * c8), dim3(256), 0, s, (const T *)a.ptr, a.stride, (const T *)b.ptr, b.stride,
                                     (T *)out.ptr, out.stride, a.n, a.h, a.w, a.c, b.h, b.w, sg, act));
    return hipGetLastError();
}

// ---- darknet letterbox_image (DN/image.c:960-981) fused with the layout change: a planar float image of any size -> px_letterbox,
//      written as the network input (whole granules per pixel) ----
template <typename T, int NCH>
__global__ void k_letterbox_chw(const float *img, int iw, int ih, int net_h, int net_w, int new_w, int new_h, int off_x, int off_y, T *out, int out_stride, int nch)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = NCH ? 0 : idx / (net_h * net_w), p = NCH ? idx : idx - g * (net_h * net_w);
    if (NCH ? p >= net_h * net_w : g * 8 >= nch) return;
    const Planes<NCH> pl(g, nch);
    const int oy = p / net_w, ox = p - oy * net_w;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    px_letterbox<NCH ? NCH : 8>(AtPlanar{img, iw, ih}, iw, ih, new_w, new_h, off_x, off_y, oy, ox, pl.c0, pl.nc, v);
    Elt<T>::store8(out + (size_t)p * out_stride + pl.c0, v);
}
hipError_t launch_letterbox_chw(const float *img, int iw, int ih, int net_h, int net_w, void *out, int out_dt, int out_stride, hipStream_t s, int nch)
{
    int new_w, new_h;
    letterbox_dims(net_w, net_h, iw, ih, &new_w, &new_h);
    const int c8 = (nch + 7) / 8;
    if (new_w < 1 || new_h < 1 || nch < 1 || out_stride < c8 * 8 || (size_t)net_h * net_w * c8 > 0x7fffffffull) return hipErrorInvalidValue;
    if (nch == 3) WITH_DT(out_dt, hipLaunchKernelGGL((k_letterbox_chw<T, 3>), grid_for((size_t)net_h * net_w), dim3(256), 0, s, img, iw, ih, net_h, net_w, new_w, new_h, (net_w - new_w) / 2, (net_h - new_h) / 2, (T *)out, out_stride, 3));
    else WITH_DT(out_dt, hipLaunchKernelGGL((k_letterbox_chw<T, 0>), grid_for((size_t)net_h * net_w * c8), dim3(256), 0, s, img, iw, ih, net_h, net_w, new_w, new_h, (net_w - new_w) / 2, (net_h - new_h) / 2, (T *)out, out_stride, nch));
    return hipGetLastError();
}

// ---- ragged batch fit (yolo_forward_images_u8): native-size uint8 RGB images packed in one HWC buffer, described by a device table of
//      {offset, h, w}, fitted into the network input [n][net_h][net_w][out_stride] by ONE launch: grid (pixel tiles) x (images), one output pixel
//      per lane, the 16-byte output pixel (8 channels: 3 real + 5 zero) stored as one vector; images of `nch` planes (NCH = 0): grid
//      (pixel tiles x granules) x (images), one output pixel x granule per lane, source pixels `nch` bytes apart.  Per pixel, each fit is the single-image
//      kernel's arithmetic (px_stretch / px_letterbox / px_cv2; px_center_crop has no single-image kernel), so a batched image equals the same image run alone, bit for bit.
//      Source bytes are read through a buffer descriptor whose size is the packed buffer's byte count: a descriptor that pointed past
//      the end would read zeros, never another allocation (the host validates every descriptor before the launch anyway).
struct AtPacked {
    __amdgpu_buffer_rsrc_t rsrc; unsigned base, pitch; int fit; unsigned px;      // pitch: bytes from one row to the next (a whole image: w * px; a window: its image's); px: bytes from one pixel to the next (the channel count)
    __device__ __forceinline__ float operator()(int y, int x, int c) const
    {
        const unsigned v = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rsrc, base + (unsigned)y * pitch + (unsigned)x * px + (unsigned)c, 0, 0);
        // STRETCH and CV2 read the byte as a float (the /255 and /225 are part of px_stretch / px_cv2); LETTERBOX, CENTER_CROP and TEN_CROP read darknet's 0..1 value
        return fit == FIT_LETTERBOX || fit == FIT_CENTER_CROP || fit == FIT_TEN_CROP ? fit_unit_value(FIT_LETTERBOX, v) : (float)v;
    }
};

__device__ __forceinline__ unsigned row_pitch(const ImgDesc &d, unsigned px) { return (unsigned)d.w * px; }
__device__ __forceinline__ unsigned row_pitch(const WinDesc &d, unsigned) { return (unsigned)d.pitch; }
__device__ __forceinline__ unsigned row_pitch(const ViewDesc &d, unsigned px) { return (unsigned)d.w * px; }
// the column of the fitted image an output column shows: a mirrored view (flip_image on the network-sized image) reads the fit at net_w - 1 - ox
template <class Desc> __device__ __forceinline__ int view_column(const Desc &, int ox, int) { return ox; }
__device__ __forceinline__ int view_column(const ViewDesc &d, int ox, int net_w) { return d.flip ? net_w - 1 - ox : ox; }
// Desc: ImgDesc (whole images), WinDesc (windows of larger images, yolo_detect_tiled_u8) or ViewDesc (one view of an image per slot, yolo_classify_views_u8):
// the same arithmetic over (h, w) pixels read at a row pitch.  FIT_TEN_CROP (ViewDesc only) mirrors inside px_ten_crop, in the resized image's coordinates
template <typename T, int FIT, class Desc, int NCH>
__global__ __launch_bounds__(256) void k_fit_images(const uint8_t *pixels, unsigned bytes, const Desc *descs, int net_h, int net_w, T *out, int out_stride,
                                                    float post_mul, float post_add, int nch, int tiles)
{
    static_assert(NCH == 3 || (FIT != FIT_CV2 && FIT != FIT_CV2_BGR), "the cv2 fits mean an RGB / BGR image");
    constexpr int NC = NCH ? NCH : 8;
    const int img = blockIdx.y;
    const int g = NCH ? 0 : blockIdx.x / tiles;          // (tiles: pixel tiles per granule, the x extent of the RGB form's grid)
    const int p = (NCH ? blockIdx.x : blockIdx.x - g * tiles) * 256 + threadIdx.x;
    if (p >= net_h * net_w) return;
    const Planes<NCH> pl(g, nch);
    const Desc d = descs[img];
    const int oy = p / net_w, ox = FIT == FIT_TEN_CROP ? p - oy * net_w : view_column(d, p - oy * net_w, net_w);
    const unsigned px = NCH ? NCH : (unsigned)nch;
    const AtPacked at{__builtin_amdgcn_make_buffer_rsrc((void *)pixels, 0, bytes, 0x00020000), (unsigned)d.offset, row_pitch(d, px), FIT, px};
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (FIT == FIT_STRETCH) px_stretch<NC>(at, d.h, d.w, net_h, net_w, oy, ox, post_mul, post_add, pl.c0, pl.nc, v);
    else {
        if (FIT == FIT_LETTERBOX) {
            int new_w, new_h;
            letterbox_dims(net_w, net_h, d.w, d.h, &new_w, &new_h);
            px_letterbox<NC>(at, d.w, d.h, new_w, new_h, (net_w - new_w) / 2, (net_h - new_h) / 2, oy, ox, pl.c0, pl.nc, v);
        } else if (FIT == FIT_CENTER_CROP) px_center_crop<NC>(at, d.w, d.h, net_w, net_h, oy, ox, pl.c0, pl.nc, v);
        else if constexpr (FIT == FIT_TEN_CROP) px_ten_crop<NC>(at, d.w, d.h, net_w, net_h, d.shift, d.dy, d.dx, d.flip, oy, ox, pl.c0, pl.nc, v);
        else if constexpr (NCH == 3) px_cv2(at, d.h, d.w, net_h, net_w, oy, ox, FIT == FIT_CV2_BGR, 225.0f, v);
        // YOLOv1's `x * 2 - 1` ([net] yolo_input_mul / yolo_input_add), as px_stretch applies it
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (NCH != 3 && c >= pl.nc) break;
            if (post_mul != 1.0f) v[c] *= post_mul;
            if (post_add != 0.0f) v[c] += post_add;
        }
    }
    Elt<T>::store8(out + ((size_t)img * net_h * net_w + p) * out_stride + pl.c0, v);
}

hipError_t launch_fit_images(const uint8_t *pixels, size_t bytes, const ImgDesc *d_descs, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                             int out_stride, float post_mul, float post_add, hipStream_t s, int nch)
{
    if (n < 1 || net_h < 1 || net_w < 1 || (size_t)net_h * net_w > 0x7fffffffull || bytes > 0xffffffffull || fit < FIT_STRETCH || fit > FIT_CENTER_CROP) return hipErrorInvalidValue;
    const int tiles = (net_h * net_w + 255) / 256;
#define FIT_LAUNCH_N(F, D, descs, NCH, grid) WITH_DT(out_dt, hipLaunchKernelGGL((k_fit_images<T, F, D, NCH>), grid, dim3(256), 0, s, pixels, (unsigned)bytes, descs, net_h, net_w, (T *)out, out_stride, post_mul, post_add, nch, tiles))
    if (nch != 3) {          // N planes: the granule folded into the grid's x; the cv2 fits are the caller's to refuse
        const int c8 = (nch + 7) / 8;
        if (nch < 1 || out_stride < c8 * 8 || (size_t)tiles * c8 > 0x7fffffffull || fit == FIT_CV2 || fit == FIT_CV2_BGR) return hipErrorInvalidValue;
        const dim3 grid_n((unsigned)(tiles * c8), (unsigned)n);
        if (fit == FIT_STRETCH) FIT_LAUNCH_N(FIT_STRETCH, ImgDesc, d_descs, 0, grid_n);
        else if (fit == FIT_LETTERBOX) FIT_LAUNCH_N(FIT_LETTERBOX, ImgDesc, d_descs, 0, grid_n);
        else FIT_LAUNCH_N(FIT_CENTER_CROP, ImgDesc, d_descs, 0, grid_n);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)tiles, (unsigned)n);
#define FIT_LAUNCH(F, D, descs) FIT_LAUNCH_N(F, D, descs, 3, grid)
    if (fit == FIT_STRETCH) FIT_LAUNCH(FIT_STRETCH, ImgDesc, d_descs);
    else if (fit == FIT_LETTERBOX) FIT_LAUNCH(FIT_LETTERBOX, ImgDesc, d_descs);
    else if (fit == FIT_CV2) FIT_LAUNCH(FIT_CV2, ImgDesc, d_descs);
    else if (fit == FIT_CV2_BGR) FIT_LAUNCH(FIT_CV2_BGR, ImgDesc, d_descs);
    else FIT_LAUNCH(FIT_CENTER_CROP, ImgDesc, d_descs);
    return hipGetLastError();
}

hipError_t launch_fit_windows(const uint8_t *pixels, size_t bytes, const WinDesc *d_wins, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                              int out_stride, float post_mul, float post_add, hipStream_t s)
{
    if (n < 1 || net_h < 1 || net_w < 1 || (size_t)net_h * net_w > 0x7fffffffull || bytes > 0xffffffffull || (fit != FIT_STRETCH && fit != FIT_LETTERBOX)) return hipErrorInvalidValue;
    const int tiles = (net_h * net_w + 255) / 256, nch = 3;
    const dim3 grid((unsigned)tiles, (unsigned)n);
    if (fit == FIT_STRETCH) FIT_LAUNCH(FIT_STRETCH, WinDesc, d_wins);
    else FIT_LAUNCH(FIT_LETTERBOX, WinDesc, d_wins);
    return hipGetLastError();
}

// the same launch over n views (yolo_classify_views_u8): slot i shows the image its descriptor names, mirrored where it says so; FIT_TEN_CROP: darknet's ten crops
hipError_t launch_fit_views(const uint8_t *pixels, size_t bytes, const ViewDesc *d_views, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                            int out_stride, float post_mul, float post_add, hipStream_t s, int nch)
{
    if (n < 1 || net_h < 1 || net_w < 1 || (size_t)net_h * net_w > 0x7fffffffull || bytes > 0xffffffffull || fit < FIT_STRETCH || fit > FIT_TEN_CROP) return hipErrorInvalidValue;
    const int tiles = (net_h * net_w + 255) / 256;
    if (nch != 3) {
        const int c8 = (nch + 7) / 8;
        if (nch < 1 || out_stride < c8 * 8 || (size_t)tiles * c8 > 0x7fffffffull || fit == FIT_CV2 || fit == FIT_CV2_BGR) return hipErrorInvalidValue;
        const dim3 grid_n((unsigned)(tiles * c8), (unsigned)n);
        if (fit == FIT_STRETCH) FIT_LAUNCH_N(FIT_STRETCH, ViewDesc, d_views, 0, grid_n);
        else if (fit == FIT_LETTERBOX) FIT_LAUNCH_N(FIT_LETTERBOX, ViewDesc, d_views, 0, grid_n);
        else if (fit == FIT_CENTER_CROP) FIT_LAUNCH_N(FIT_CENTER_CROP, ViewDesc, d_views, 0, grid_n);
        else FIT_LAUNCH_N(FIT_TEN_CROP, ViewDesc, d_views, 0, grid_n);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)tiles, (unsigned)n);
    if (fit == FIT_STRETCH) FIT_LAUNCH(FIT_STRETCH, ViewDesc, d_views);
    else if (fit == FIT_LETTERBOX) FIT_LAUNCH(FIT_LETTERBOX, ViewDesc, d_views);
    else if (fit == FIT_CV2) FIT_LAUNCH(FIT_CV2, ViewDesc, d_views);
    else if (fit == FIT_CV2_BGR) FIT_LAUNCH(FIT_CV2_BGR, ViewDesc, d_views);
    else if (fit == FIT_CENTER_CROP) FIT_LAUNCH(FIT_CENTER_CROP, ViewDesc, d_views);
    else FIT_LAUNCH(FIT_TEN_CROP, ViewDesc, d_views);
#undef FIT_LAUNCH
#undef FIT_LAUNCH_N
    return hipGetLastError();
}

// ---- decoded video frames (yolo_*_frames_*; kernels.h FrameDesc): the source reader of a frame.  at(y, x, c) is byte c of the h x w x 3 image the colour rule
//      yields at pixel (y0 + y, x0 + x) of the frame -- (y0, x0): where a window begins, 0 for a whole frame; chroma is indexed in the FRAME -- as AtPacked returns it
//      for a packed RGB image, so every px_* fit above runs over it unchanged.  The conversion is integer-exact: how often a tap's three channels evaluate it cannot
//      change a bit, and the compiler folds the three evaluations of one tap into one (the loads are the same addresses; NOTEBOOK 2026-10-21).  Format and matrix
//      are the frame's: uniform over a workgroup (blockIdx.y is the frame), so one batch may mix them.
struct AtFrame {
    __amdgpu_buffer_rsrc_t rsrc; FrameDesc f; ColorMatrix m; int y0, x0, fit;
    __device__ __forceinline__ unsigned byte_at(unsigned off) const { return (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rsrc, off, 0, 0); }
    __device__ __forceinline__ void rgb(int y, int x, int *v) const
    {
        // a decoded JPEG file: luma direct, chroma through the reference's upsampler at the pixel's position in the frame, the reference's colour step (kernels.h)
        if (pix_is_jpeg(f.format)) { jpeg_frame_rgb(f, y0 + y, x0 + x, [&](unsigned off) { return (int)byte_at(off); }, v); return; }
        unsigned o[3];
        frame_sample_offsets(f, y0 + y, x0 + x, o);
        const int a = (int)byte_at(o[0]), b = (int)byte_at(o[1]), c = (int)byte_at(o[2]);
        if (f.format >= PIX_RGB24) { v[0] = a; v[1] = b; v[2] = c; }
        else yuv_to_rgb(m, a, b, c, v);
    }
    __device__ __forceinline__ float operator()(int y, int x, int c) const
    {
        int v[3];
        rgb(y, x, v);
        const unsigned b = (unsigned)(c == 0 ? v[0] : c == 1 ? v[1] : v[2]);
        return fit == FIT_LETTERBOX || fit == FIT_CENTER_CROP || fit == FIT_TEN_CROP ? fit_unit_value(FIT_LETTERBOX, b) : (float)b;
    }
};

// k_fit_images over frames.  What a batch slot shows: frame i itself; window wins[i] of frame wins[i].image (slots: the WinDesc table); or one view of frame
// views[i].offset (slots: the ViewDesc table, whose `offset` field holds the FRAME INDEX here, h and w the frame's), with k_fit_images<.., ViewDesc, 3>'s meaning:
// a mirrored view reads the fit at view_column, FIT_TEN_CROP crops and mirrors in the resized image's coordinates.  A view's pixels are pixels of the whole frame
// (y0 = x0 = 0), so its chroma is indexed in the frame whatever the mirror or the crop does
enum { SLOT_FRAME = 0, SLOT_WINDOW = 1, SLOT_VIEW = 2 };
template <typename T, int FIT, int SLOT>
__global__ __launch_bounds__(256) void k_fit_frames(const uint8_t *pixels, unsigned bytes, const FrameDesc *frames, const void *slots, int net_h, int net_w, T *out,
                                                    int out_stride, float post_mul, float post_add)
{
    static_assert(FIT != FIT_TEN_CROP || SLOT == SLOT_VIEW, "the ten crops are views");
    const int img = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= net_h * net_w) return;
    int h = 0, w = 0, y0 = 0, x0 = 0, fi = img;
    ViewDesc view = {};
    if (SLOT == SLOT_WINDOW) { const WinDesc d = ((const WinDesc *)slots)[img]; h = d.h; w = d.w; y0 = d.y0; x0 = d.x0; fi = d.image; }
    if (SLOT == SLOT_VIEW) { view = ((const ViewDesc *)slots)[img]; fi = (int)view.offset; }
    const FrameDesc f = frames[fi];
    if (SLOT != SLOT_WINDOW) { h = f.h; w = f.w; }
    const int oy = p / net_w, ox = SLOT == SLOT_VIEW && FIT != FIT_TEN_CROP ? view_column(view, p - oy * net_w, net_w) : p - oy * net_w;
    const AtFrame at{__builtin_amdgcn_make_buffer_rsrc((void *)pixels, 0, bytes, 0x00020000), f, color_matrix(f.matrix), y0, x0, FIT};
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (FIT == FIT_STRETCH) px_stretch<3>(at, h, w, net_h, net_w, oy, ox, post_mul, post_add, 0, 3, v);
    else {
        if (FIT == FIT_LETTERBOX) {
            int new_w, new_h;
            letterbox_dims(net_w, net_h, w, h, &new_w, &new_h);
            px_letterbox<3>(at, w, h, new_w, new_h, (net_w - new_w) / 2, (net_h - new_h) / 2, oy, ox, 0, 3, v);
        } else if (FIT == FIT_CENTER_CROP) px_center_crop<3>(at, w, h, net_w, net_h, oy, ox, 0, 3, v);
        else if constexpr (FIT == FIT_TEN_CROP) px_ten_crop<3>(at, w, h, net_w, net_h, view.shift, view.dy, view.dx, view.flip, oy, ox, 0, 3, v);
        else px_cv2(at, h, w, net_h, net_w, oy, ox, 0, 225.0f, v);
        // [net] yolo_input_mul / yolo_input_add, as k_fit_images applies them
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (post_mul != 1.0f) v[c] *= post_mul;
            if (post_add != 0.0f) v[c] += post_add;
        }
    }
    Elt<T>::store8(out + ((size_t)img * net_h * net_w + p) * out_stride, v);
}

// slots: the WinDesc table (SLOT_WINDOW: FIT_STRETCH, FIT_LETTERBOX), the ViewDesc table (SLOT_VIEW: every fit of whole frames, and FIT_TEN_CROP), NULL for whole frames
static hipError_t fit_frames(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, const void *slots, int slot, int n, int fit, int net_h, int net_w, void *out,
                             int out_dt, int out_stride, float post_mul, float post_add, hipStream_t s)
{
    if (n < 1 || net_h < 1 || net_w < 1 || (size_t)net_h * net_w > 0x7fffffffull || bytes > 0xffffffffull || out_stride < 8 || (slot != SLOT_FRAME) != (slots != nullptr)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((net_h * net_w + 255) / 256), (unsigned)n);
#define FRAMES_LAUNCH(F, SLOT) WITH_DT(out_dt, hipLaunchKernelGGL((k_fit_frames<T, F, SLOT>), grid, dim3(256), 0, s, pixels, (unsigned)bytes, d_frames, slots, net_h, net_w, (T *)out, out_stride, post_mul, post_add))
    if (slot == SLOT_WINDOW) {
        if (fit == FIT_STRETCH) FRAMES_LAUNCH(FIT_STRETCH, SLOT_WINDOW);
        else if (fit == FIT_LETTERBOX) FRAMES_LAUNCH(FIT_LETTERBOX, SLOT_WINDOW);
        else return hipErrorInvalidValue;
    } else if (slot == SLOT_VIEW) {
        if (fit == FIT_STRETCH) FRAMES_LAUNCH(FIT_STRETCH, SLOT_VIEW);
        else if (fit == FIT_LETTERBOX) FRAMES_LAUNCH(FIT_LETTERBOX, SLOT_VIEW);
        else if (fit == FIT_CV2) FRAMES_LAUNCH(FIT_CV2, SLOT_VIEW);
        else if (fit == FIT_CENTER_CROP) FRAMES_LAUNCH(FIT_CENTER_CROP, SLOT_VIEW);
        else if (fit == FIT_TEN_CROP) FRAMES_LAUNCH(FIT_TEN_CROP, SLOT_VIEW);
        else return hipErrorInvalidValue;
    } else if (fit == FIT_STRETCH) FRAMES_LAUNCH(FIT_STRETCH, SLOT_FRAME);
    else if (fit == FIT_LETTERBOX) FRAMES_LAUNCH(FIT_LETTERBOX, SLOT_FRAME);
    else if (fit == FIT_CV2) FRAMES_LAUNCH(FIT_CV2, SLOT_FRAME);
    else if (fit == FIT_CENTER_CROP) FRAMES_LAUNCH(FIT_CENTER_CROP, SLOT_FRAME);
    else return hipErrorInvalidValue;
#undef FRAMES_LAUNCH
    return hipGetLastError();
}
hipError_t launch_fit_frames(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                             int out_stride, float post_mul, float post_add, hipStream_t s)
{
    return fit_frames(pixels, bytes, d_frames, nullptr, SLOT_FRAME, n, fit, net_h, net_w, out, out_dt, out_stride, post_mul, post_add, s);
}
hipError_t launch_fit_frame_windows(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, const WinDesc *d_wins, int n, int fit, int net_h, int net_w,
                                    void *out, int out_dt, int out_stride, float post_mul, float post_add, hipStream_t s)
{
    return fit_frames(pixels, bytes, d_frames, d_wins, SLOT_WINDOW, n, fit, net_h, net_w, out, out_dt, out_stride, post_mul, post_add, s);
}
hipError_t launch_fit_frame_views(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, const ViewDesc *d_views, int n, int fit, int net_h, int net_w,
                                  void *out, int out_dt, int out_stride, float post_mul, float post_add, hipStream_t s)
{
    return fit_frames(pixels, bytes, d_frames, d_views, SLOT_VIEW, n, fit, net_h, net_w, out, out_dt, out_stride, post_mul, post_add, s);
}

// one frame -> [h][w][3] uint8: the colour rule by itself (yolo_op_frame_to_rgb); one pixel per lane
__global__ __launch_bounds__(256) void k_frame_to_rgb(const uint8_t *pixels, unsigned bytes, FrameDesc f, uint8_t *out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)f.h * f.w) return;
    const int y = (int)(p / f.w), x = (int)(p - (size_t)y * f.w);
    const AtFrame at{__builtin_amdgcn_make_buffer_rsrc((void *)pixels, 0, bytes, 0x00020000), f, color_matrix(f.matrix), 0, 0, FIT_CV2};
    int v[3];
    at.rgb(y, x, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (uint8_t)v[c];
}
hipError_t launch_frame_to_rgb(const uint8_t *pixels, size_t bytes, const FrameDesc &frame, uint8_t *out, hipStream_t s)
{
    if (frame.h < 1 || frame.w < 1 || bytes > 0xffffffffull || frame.format < 0 || (frame.format >= PIX_COUNT && !pix_is_jpeg(frame.format)) || frame.matrix < 0 || frame.matrix >= MATRIX_COUNT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_frame_to_rgb, grid_for((size_t)frame.h * frame.w), dim3(256), 0, s, pixels, (unsigned)bytes, frame, out);
    return hipGetLastError();
}

// ---- darknet letterbox_image (DN/image.c:960-981: resize_image to the aspect-preserving size, embedded in a 0.5-grey w x h
//      canvas) and resize_image itself (DN/image.c:1347-1389; embed == 0: the image is stretched to w x h), planar float in,
//      planar float out.  Same two-pass operation order as k_letterbox_chw above. ----
__global__ void k_letterbox_planar(const float *img, int iw, int ih, int W, int H, int new_w, int new_h, int off_x, int off_y, float *out)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W * H) return;
    const int oy = p / W, ox = p - oy * W;
    float v[3];
    px_letterbox<3>(AtPlanar{img, iw, ih}, iw, ih, new_w, new_h, off_x, off_y, oy, ox, 0, 3, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)k * W * H + p] = v[k];
}
hipError_t launch_letterbox_planar(const float *img, int iw, int ih, int w, int h, int embed, float *out, hipStream_t s)
{
    int new_w = w, new_h = h;
    if (embed) { if (((float)w / iw) < ((float)h / ih)) { new_w = w; new_h = (ih * w) / iw; } else { new_h = h; new_w = (iw * h) / ih; } }
    if (new_w < 1 || new_h < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_letterbox_planar, grid_for((size_t)w * h), dim3(256), 0, s, img, iw, ih, w, h, new_w, new_h, (w - new_w) / 2, (h - new_h) / 2, out);
    return hipGetLastError();
}

// ---- [local]: locally connected layer (DN/local_layer.c:91-120): a conv whose filters are NOT shared between output locations.
//      out[n, oy, ox, f] = act(bias[loc][f] + sum_{kh,kw,c} W[loc][f][kh][kw][c] * in[n, oy s - p + kh, ox s - p + kw, c]), loc = oy Wo + ox.
//      Every filter value is used once per image: the layer streams its weights (darknet's yolov1.cfg: 49 locations x 256 x 9216) and
//      is HBM-bound by construction.  One wave per (location, filter): lanes run along the 8-channel granules of a tap (16-byte loads
//      of filter and activation), fp32 accumulation, shuffle reduction; the image loop is inside so the filter row is read once. ----
template <typename T>
__global__ __launch_bounds__(256) void k_local(const T *in, int in_stride, const T *w, const float *bias, T *out, int out_stride,
                                               int n, int H, int W, int C, int Ho, int Wo, int F, int k, int stride, int pad, int act)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int loc = blockIdx.x, f = blockIdx.y * 4 + wv;
    if (f >= F) {                // channels F .. roundup(F, 8) of the stored pixel: zero, so that a consumer's zero filters never meet stale Inf / NaN
        if (f < ((F + 7) & ~7) && lane == 0) for (int b = 0; b < n; ++b) Elt<T>::store1(out + ((size_t)b * Ho * Wo + loc) * out_stride + f, 0.f);
        return;
    }
    const int oy = loc / Wo, ox = loc - oy * Wo;
    const int c8n = C / 8, K8 = k * k * c8n;                      // 8-channel granules per tap / per filter row
    const T *wr = w + ((size_t)loc * F + f) * (size_t)K8 * 8;
    for (int b = 0; b < n; ++b) {
        float acc = 0.f;
        for (int g = lane; g < K8; g += 64) {
            const int t = g / c8n, c8 = g - t * c8n;
            const int kh = t / k, kw = t - kh * k;
            const int iy = oy * stride - pad + kh, ix = ox * stride - pad + kw;
            if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
            float xv[8], wv8[8];
            Elt<T>::load8(in + ((size_t)(b * H + iy) * W + ix) * in_stride + c8 * 8, xv);
            Elt<T>::load8(wr + (size_t)g * 8, wv8);
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = fmaf(xv[q], wv8[q], acc);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) {
            float v = acc + bias[(size_t)loc * F + f];
            if (act != ACT_LINEAR) v = fmaxf(v, v * act_slope(act));          // == v > 0 ? v : slope * v
            Elt<T>::store1(out + ((size_t)b * Ho * Wo + loc) * out_stride + f, v);
        }
    }
}

hipError_t launch_local(const TView &in, const TView &out, const void *w, const float *bias, int k, int stride, int pad, int act, hipStream_t s)
{
    if (in.c % 8 || in.dt != out.dt || in.dt == DT_FP8) return hipErrorInvalidValue;
    dim3 grid((unsigned)(out.h * out.w), (unsigned)((((out.c + 7) & ~7) + 3) / 4));
    WITH_DT(in.dt, hipLaunchKernelGGL(k_local<T>, grid, dim3(256), 0, s, (const T *)in.ptr, in.stride, (const T *)w, bias, (T *)out.ptr, out.stride,
                                      in.n, in.h, in.w, in.c, out.h, out.w, out.c, k, stride, pad, act));
    return hipGetLastError();
}
