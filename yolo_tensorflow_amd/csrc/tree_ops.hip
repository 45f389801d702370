// Hierarchical softmax for gfx950: darknet's softmax trees (YOLO9000's WordNet tree, the tree classifiers).  What the reference does
// on the host after pulling the layer output back (DN/tree.c:37-81 hierarchy_predictions / hierarchy_top_prediction,
// DN/region_layer.c:412-424) and in softmax_tree (DN/blas_kernels.cu, one thread per group) runs here as:
//   k_tree_softmax          one workgroup per row: waves take groups, lanes stride over members; optionally the absolute form
//                           (level by level from the root, every value cond[j] * abs[parent[j]] exactly), the leaves mask, top-k
//   k_decode_region_tree    the tree twin of k_decode_region: det rows with absolute class probabilities
//   k_tree_score_rows       scores / labels of decoded rows: objectness and hierarchy_top_prediction over the absolute values
//   k_decode_region_tree_lean / k_tree_top   the descent form: one wave per box walks from the root over the RAW logits, one group's
//                           softmax per step -- work ~ kept boxes x path length, not rows x classes
// Both forms take a group's (max, sum) from group_stats and a member's probability from group_prob, and both scale by the parent's
// absolute value with one multiplication: they produce the same bits, hence the same labels.  Built with -ffp-contract=off.
#include "kernels.h"
#include "wave_ops.h"
#include <math.h>

namespace {

constexpr int TR_NT = 256, TR_NW = TR_NT / 64;

__device__ __forceinline__ const float *row_logits(const TreeRows &x, size_t r)
{
    return x.x + (r / x.na) * (size_t)x.cell_stride + (r % x.na) * (size_t)x.an_stride + x.off;
}

// one wave: largest logit and sum of e = exp(x / t - largest / t) over the group [off, off + sz) (DN/blas.c:305-321)
__device__ __forceinline__ void group_stats(const float *x, int off, int sz, float temp, int lane, float &largest, float &sum)
{
    float m = -INFINITY;
    for (int i = lane; i < sz; i += 64) m = fmaxf(m, x[off + i]);
    largest = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < sz; i += 64) s += expf(x[off + i] / temp - largest / temp);
    sum = wave_sum(s);
}
__device__ __forceinline__ float group_prob(float xv, float temp, float largest, float sum) { return expf(xv / temp - largest / temp) / sum; }

// One row, called by every thread of a TR_NT workgroup: conditional probabilities of the n logits at x to out[j * os]; from
// TREE_ABSOLUTE on the ascending parent product, reproduced level by level; TREE_LEAVES: inner nodes zeroed.  Returns with the
// workgroup's writes not yet ordered: callers that read `out` afterwards synchronise.
__device__ void row_tree_probs(const TreeDev &t, const float *x, float temp, int mode, float *out, size_t os)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int g = wv; g < t.groups; g += TR_NW) {
        const int off = t.goff[g], sz = t.gsize[g];
        float largest, sum;
        group_stats(x, off, sz, temp, lane, largest, sum);
        for (int i = lane; i < sz; i += 64) out[(size_t)(off + i) * os] = group_prob(x[off + i], temp, largest, sum);
    }
    if (mode == TREE_CONDITIONAL) return;
    for (int L = 1; L < t.levels; ++L) {
        __syncthreads();            // the level above is complete (workgroup-scope release / acquire of the global writes)
        for (int k = t.lvl[L] + wv; k < t.lvl[L + 1]; k += TR_NW) {
            const int g = t.order[k], off = t.goff[g], sz = t.gsize[g];
            const float pa = out[(size_t)t.parent[off] * os];
            for (int i = lane; i < sz; i += 64) out[(size_t)(off + i) * os] = out[(size_t)(off + i) * os] * pa;
        }
    }
    if (mode == TREE_LEAVES) {
        __syncthreads();
        for (int j = threadIdx.x; j < t.n; j += TR_NT) if (!t.leaf[j]) out[(size_t)j * os] = 0.f;
    }
}

// hierarchy_top_prediction (DN/tree.c:53-81) by one wave, as the reference writes it: per group the first strict maximum from
// max = 0, max_i = 0; descend while p * max > thresh with p = p * max (the absolutes compound: that is what the code does); a failed
// test returns max_i at the root group and the group's parent node deeper down.  VALUE(off + i): the absolute probability of a node
template <typename Value>
__device__ __forceinline__ int wave_tree_walk(const TreeDev &t, float thresh, int lane, Value value)
{
    float p = 1.f, pabs = 1.f;
    int group = 0;
    for (;;) {
        const int off = t.goff[group], sz = t.gsize[group];
        float best = 0.f; int bi = 0x7fffffff;
        value(off, sz, pabs, best, bi);
        wave_argmax(best, bi);
        if (bi == 0x7fffffff) bi = 0;              // nothing above 0: max_i keeps its initial 0
        if (p * best > thresh) {
            p = p * best;
            group = t.child[bi];
            if (group < 0) return bi;
            pabs = best;
        } else return group == 0 ? bi : t.parent[off];
    }
}
// ... over stored absolute probabilities a[0 .. n)
__device__ __forceinline__ int wave_tree_top_abs(const TreeDev &t, const float *a, float thresh, int lane)
{
    return wave_tree_walk(t, thresh, lane, [&](int off, int sz, float, float &best, int &bi) {
        for (int i = lane; i < sz; i += 64) first_max(best, bi, a[off + i], off + i);
    });
}
// ... over raw logits (temperature 1): the group's softmax on the way, scaled by the parent's absolute value
__device__ __forceinline__ int wave_tree_top_raw(const TreeDev &t, const float *x, float thresh, int lane)
{
    return wave_tree_walk(t, thresh, lane, [&](int off, int sz, float pabs, float &best, int &bi) {
        float largest, sum;
        group_stats(x, off, sz, 1.f, lane, largest, sum);
        for (int i = lane; i < sz; i += 64) first_max(best, bi, group_prob(x[off + i], 1.f, largest, sum) * pabs, off + i);
    });
}

// the best top_k of p[0 .. n) in the order of classify()'s stable sort; round r takes the best entry that ranks after round r - 1's
__device__ void row_topk(const float *p, int n, int top_k, int *cls, float *tkp, float *red_p, int *red_i)
{
    const int t = threadIdx.x;
    float prev_p = 0.f; int prev_i = -1; bool done = false;
    for (int r = 0; r < top_k; ++r) {
        float bp = 0.f; int bi = -1;
        if (!done)
            for (int j = t; j < n; j += TR_NT) {
                const float q = p[j];
                const bool after = prev_i < 0 || q < prev_p || (q == prev_p && j > prev_i);
                if (after && ranks_before(q, j, bp, bi)) { bp = q; bi = j; }
            }
        block_best(bp, bi, red_p, red_i);
        if (t == 0) { cls[r] = bi; tkp[r] = bi >= 0 ? bp : 0.f; }
        if (bi < 0) done = true;
        prev_p = bp; prev_i = bi;
    }
}

__global__ __launch_bounds__(TR_NT) void k_tree_softmax(const TreeDev t, const TreeRows x, float temp, int mode, float *out, int out_stride,
                                                        int top_k, int *cls, float *tkp)
{
    __shared__ float red_p[TR_NW];
    __shared__ int red_i[TR_NW];
    const size_t r = blockIdx.x;
    float *o = out + r * (size_t)out_stride;
    row_tree_probs(t, row_logits(x, r), temp, mode, o, 1);
    if (top_k > 0) { __syncthreads(); row_topk(o, t.n, top_k, cls + r * top_k, tkp + r * top_k, red_p, red_i); }
}

__global__ __launch_bounds__(TR_NT) void k_tree_top(const TreeDev t, const TreeRows x, float thresh, int *labels)
{
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * TR_NW + (threadIdx.x >> 6);
    if (r >= x.rows) return;
    const int j = wave_tree_top_raw(t, row_logits(x, r), thresh, lane);
    if (lane == 0) labels[r] = j;
}

// box `box` of the head: its raw values, its cell and anchor, its row in the decoded tensor
struct RegionBox { const float *p; int cell, an; size_t row; };
__device__ __forceinline__ RegionBox region_box_of(const DecodeArgs &a, size_t box)
{
    RegionBox b;
    b.an = (int)(box % a.na); const size_t c = box / a.na;
    const size_t gg = (size_t)a.gh * a.gw;
    b.cell = (int)(c % gg); const size_t img = c / gg;
    b.p = a.raw + (img * gg + b.cell) * (size_t)a.raw_stride + (size_t)b.an * (5 + a.classes);
    b.row = img * a.rows_total + a.row_off + (size_t)b.cell * a.na + b.an;
    return b;
}

__global__ __launch_bounds__(TR_NT) void k_decode_region_tree(const DecodeArgs a, const TreeDev t)
{
    const RegionBox b = region_box_of(a, blockIdx.x);
    float *o = a.det + b.row * (size_t)(5 + a.classes);
    if (threadIdx.x < 5) o[threadIdx.x] = region_box_attr(threadIdx.x, b.p, b.cell, a.gw, a.gh, a.anchors + 2 * b.an);
    row_tree_probs(t, b.p + 5, 1.f, TREE_ABSOLUTE, o + 5, 1);
}

__global__ __launch_bounds__(TR_NT) void k_tree_score_rows(const float *det, size_t nrows, int attrs, const TreeDev t, float thresh, float *scores, int *labels)
{
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * TR_NW + (threadIdx.x >> 6);
    if (r >= nrows) return;
    const float *p = det + r * (size_t)attrs;
    const int j = wave_tree_top_abs(t, p + 5, thresh, lane);
    if (lane == 0) { scores[r] = p[4]; labels[r] = j; }
}

__global__ __launch_bounds__(TR_NT) void k_decode_region_tree_lean(const DecodeArgs a, const TreeDev t, float thresh, float *scores, int *labels)
{
    const int lane = threadIdx.x & 63;
    const size_t box = (size_t)blockIdx.x * TR_NW + (threadIdx.x >> 6), total = (size_t)a.n * a.gh * a.gw * a.na;
    if (box >= total) return;
    const RegionBox b = region_box_of(a, box);
    if (lane < 4) a.box4[b.row * 4 + lane] = region_box_attr(lane, b.p, b.cell, a.gw, a.gh, a.anchors + 2 * b.an);
    const float obj = region_box_attr(4, b.p, b.cell, a.gw, a.gh, a.anchors + 2 * b.an);
    int j = 0;
    if (obj >= a.reject_below) j = wave_tree_top_raw(t, b.p + 5, thresh, lane);      // (wave-uniform: every lane holds the same objectness)
    if (lane == 0) { scores[b.row] = obj; labels[b.row] = j; }
}

__global__ __launch_bounds__(TR_NT) void k_darknet_tree_probs(const float *det, int attrs, const TreeDev t, float thresh, float hier_thresh,
                                                              const int *map200, float *rec, const int *src, const int *count, int cap)
{
    const int n = *count < cap ? *count : cap;
    if ((int)blockIdx.x >= n) return;
    const float *p = det + (size_t)src[blockIdx.x] * attrs;
    float *o = rec + (size_t)blockIdx.x * attrs + 5;
    const float scale = p[4];
    const int classes = attrs - 5;
    if (map200) {
        for (int j = threadIdx.x; j < classes; j += TR_NT) {
            float v = 0.f;
            if (j < 200) { const float prob = scale * p[5 + map200[j]]; v = prob > thresh ? prob : 0.f; }
            o[j] = v;
        }
        return;
    }
    const int top = wave_tree_top_abs(t, p + 5, hier_thresh, threadIdx.x & 63);      // (every wave walks: the same result in all four)
    for (int j = threadIdx.x; j < classes; j += TR_NT) o[j] = (j == top && scale > thresh) ? scale : 0.f;
}

__global__ __launch_bounds__(TR_NT) void k_head_darknet_layout_tree(const float *raw, int raw_stride, int cells, int na, int classes, const TreeDev t, float *out)
{
    const int r = blockIdx.x, cell = r / na, n = r - cell * na, attrs = 5 + classes;
    const float *p = raw + (size_t)cell * raw_stride + n * attrs;
    float *o = out + (size_t)n * attrs * cells + cell;
    if (threadIdx.x < 5) o[(size_t)threadIdx.x * cells] = darknet_layout_box_attr(threadIdx.x, p);
    row_tree_probs(t, p + 5, 1.f, TREE_CONDITIONAL, o + (size_t)5 * cells, (size_t)cells);
}

bool tree_ok(const TreeDev &t) { return t.n >= 1 && t.groups >= 1 && t.levels >= 1 && t.parent && t.child && t.goff && t.gsize && t.leaf && t.order && t.lvl; }

}  // namespace

hipError_t launch_tree_softmax(const TreeDev &t, const TreeRows &x, float temperature, int mode, float *out, int out_stride,
                               int top_k, int *cls, float *topk_probs, hipStream_t s)
{
    if (!tree_ok(t) || !x.x || x.rows < 1 || x.rows > 0x7fffffffull || x.na < 1 || !out || out_stride < t.n || !(temperature > 0.f)) return hipErrorInvalidValue;
    if (mode < TREE_CONDITIONAL || mode > TREE_LEAVES || top_k < 0 || top_k > CLS_TOPK_MAX || (top_k > 0 && (!cls || !topk_probs))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tree_softmax, dim3((unsigned)x.rows), dim3(TR_NT), 0, s, t, x, temperature, mode, out, out_stride, top_k, cls, topk_probs);
    return hipGetLastError();
}

hipError_t launch_tree_top(const TreeDev &t, const TreeRows &x, float hier_thresh, int *labels, hipStream_t s)
{
    if (!tree_ok(t) || !x.x || x.rows < 1 || x.rows > 0x7fffffffull || x.na < 1 || !labels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tree_top, dim3((unsigned)((x.rows + TR_NW - 1) / TR_NW)), dim3(TR_NT), 0, s, t, x, hier_thresh, labels);
    return hipGetLastError();
}

static bool region_tree_args_ok(const DecodeArgs &a, const TreeDev &t)
{
    const size_t total = (size_t)a.n * a.gh * a.gw * a.na;
    return tree_ok(t) && a.raw && a.region && t.n == a.classes && a.n >= 1 && a.gh >= 1 && a.gw >= 1 && a.na >= 1 && a.na <= 16 && a.raw_stride >= a.na * (5 + a.classes) && total <= 0x7fffffffull;
}

hipError_t launch_decode_region_tree(const DecodeArgs &a, const TreeDev &t, hipStream_t s)
{
    if (!region_tree_args_ok(a, t) || !a.det) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_decode_region_tree, dim3((unsigned)((size_t)a.n * a.gh * a.gw * a.na)), dim3(TR_NT), 0, s, a, t);
    return hipGetLastError();
}

hipError_t launch_tree_score_rows(const float *det, size_t nrows, int attrs, const TreeDev &t, float hier_thresh, float *scores, int *labels, hipStream_t s)
{
    if (!tree_ok(t) || !det || nrows < 1 || nrows > 0x7fffffffull || attrs != 5 + t.n || !scores || !labels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tree_score_rows, dim3((unsigned)((nrows + TR_NW - 1) / TR_NW)), dim3(TR_NT), 0, s, det, nrows, attrs, t, hier_thresh, scores, labels);
    return hipGetLastError();
}

hipError_t launch_decode_region_tree_lean(const DecodeArgs &a, const TreeDev &t, float hier_thresh, float *scores, int *labels, hipStream_t s)
{
    if (!region_tree_args_ok(a, t) || !a.box4 || !scores || !labels) return hipErrorInvalidValue;
    const size_t total = (size_t)a.n * a.gh * a.gw * a.na;
    hipLaunchKernelGGL(k_decode_region_tree_lean, dim3((unsigned)((total + TR_NW - 1) / TR_NW)), dim3(TR_NT), 0, s, a, t, hier_thresh, scores, labels);
    return hipGetLastError();
}

hipError_t launch_darknet_tree_probs(const float *det, int attrs, const TreeDev &t, float thresh, float hier_thresh, const int *map200,
                                     float *rec, const int *src, const int *count, int cap, hipStream_t s)
{
    if (!tree_ok(t) || !det || attrs != 5 + t.n || !rec || !src || !count || cap < 1 || (map200 && t.n < 200)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_darknet_tree_probs, dim3((unsigned)cap), dim3(TR_NT), 0, s, det, attrs, t, thresh, hier_thresh, map200, rec, src, count, cap);
    return hipGetLastError();
}

hipError_t launch_head_darknet_layout_tree(const float *raw, int raw_stride, int cells, int na, int classes, const TreeDev &t, float *out, hipStream_t s)
{
    if (!tree_ok(t) || !raw || !out || cells < 1 || na < 1 || classes != t.n || raw_stride < na * (5 + classes)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_head_darknet_layout_tree, dim3((unsigned)(cells * na)), dim3(TR_NT), 0, s, raw, raw_stride, cells, na, classes, t, out);
    return hipGetLastError();
}
