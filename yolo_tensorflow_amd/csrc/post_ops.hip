// Detection-head post-processing on the device (the reference has NO GPU kernel for this: darknet pulls
// the head tensor to the host, DN/yolo_layer.c:347-362, and runs DN/box.c on the CPU; the TF scripts run
// tf.boolean_mask / tf.image.non_max_suppression or pure-numpy loops, V3/yolo_v3.py:376-420).
//
//   k_decode_yolo* / k_decode_region: rows D3 / D2 -- raw head conv output -> [n, rows, 5+C] fp32
//   k_score_rows                    : row S        -- score = max_k(obj*cls_k), label = first argmax
//   k_nms_image (1 workgroup/image) : rows S+N     -- order-preserving threshold compaction, sort by
//                                     score (ties: lower row first), greedy suppression, top max_out
//
// Built with -ffp-contract=off: every IoU is evaluated with the reference's operation order in fp32
// (or fp64 for the V2 numpy flavour) so the kept set is bit-identical to the oracle on equal inputs.
#include "kernels.h"
#include "wave_ops.h"
#include <math.h>

struct BoxOut { float x0, y0, x1, y1, score; int cls; };

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// hardware-rate sigmoid for the 83 of 85 attributes that are probabilities: v_exp_f32 (2^x, 1 ulp) on x*log2(e) and
// v_rcp_f32 (1 ulp).  |rel err| <= ~1.2e-6 for |x| <= 20 (the rounding of x*log2e), inside the 3e-6 the decode is
// tested to; box sizes keep the full-precision expf.
__device__ __forceinline__ float sigmoid_fast(float x)
{
    const float e = __builtin_amdgcn_exp2f(-x * 1.44269504088896340736f);
    return __builtin_amdgcn_rcpf(1.0f + e);
}

// Attribute k (0 x, 1 y, 2 w, 3 h) of a [yolo] box, the ONE place this arithmetic is written (`_detection_layer`, V3/yolo_v3.py:111-159, and
// `_ratio_detection_layer`, V3/YOLOV3.py:168-238): x raw value, (cx, cy) grid cell, anchor = the box's (w, h) pair pre-divided by the
// stride on the host, (GW, GH) grid columns and rows, (SX, SY) the strides along x and y: x and w take GW / SX, y and h GH / SY (one value
// each on a square network).  mode 0 divides by G, the pixel mode multiplies by S: not interchangeable without contraction, and the
// operand order is the reference's.
// It is written in two steps: yolo_box_act, the value darknet's [yolo] layer holds in l.output (logistic on x and y, w and h raw), and yolo_box_form, the
// box formula on such a value.  The frame-averaged decode (k_decode_avg<false>) takes the mean of activated values between the two.
__device__ __forceinline__ float yolo_box_act(int k, float x) { return k < 2 ? sigmoidf_(x) : x; }
__device__ __forceinline__ float yolo_box_form(int k, float v, int cx, int cy, const float *anchor, float GW, float GH, float SX, float SY, int mode)
{
    const float t = k < 2 ? v + (float)(k == 0 ? cx : cy) : expf(v) * anchor[k - 2];
    const float G = (k & 1) ? GH : GW, S = (k & 1) ? SY : SX;
    return mode == 0 ? t / G : t * S;
}
__device__ __forceinline__ float yolo_box_attr(int k, float x, int cx, int cy, const float *anchor, float GW, float GH, float SX, float SY, int mode)
{
    return yolo_box_form(k, yolo_box_act(k, x), cx, cy, anchor, GW, GH, SX, SY, mode);
}

// ---- D3 (+S): `_detection_layer` (V3/yolo_v3.py:111-159) / `_ratio_detection_layer` (V3/YOLOV3.py:168-238),
//      fused with the row score of V3/YOLOV3.py:353-357.  One wave per candidate box: lanes run along the
//      5+C attributes (contiguous in the head tensor and in the decoded tensor -> fully coalesced), the
//      max/argmax over classes is a wave shuffle reduction. ----
__global__ __launch_bounds__(256) void k_decode_yolo(const DecodeArgs a, float *scores, int *labels)
{
    const int attrs = 5 + a.classes;
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    const int gg = a.gh * a.gw;
    const long total = (long)a.n * gg * a.na;
    const float GW = (float)a.gw, GH = (float)a.gh, SX = (float)(a.img_w / a.gw), SY = (float)(a.img_h / a.gh);
    constexpr int U = 4;                       // boxes in flight per wave (memory-level parallelism)
    const bool two = attrs > 64;               // second 64-attribute pass needed (attrs <= 128 is enforced by the launcher)
    for (long b0 = wave * U; b0 < total; b0 += nwaves * U) {
        float v0[U], v1[U];
        const float *src[U]; float *dst[U]; size_t rowi[U]; int an_[U], cell_[U];
        // (image, cell, anchor) of the first box by 32-bit division, the next three by increment: the index math is
        // wave-uniform and must stay far cheaper than the 85 sigmoids it serves
        const unsigned ub = (unsigned)__builtin_amdgcn_readfirstlane((int)b0);
        unsigned t0 = ub / (unsigned)a.na; int an = (int)(ub - t0 * a.na);
        int b = (int)(t0 / (unsigned)gg); int cell = (int)(t0 - (unsigned)b * gg);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u > 0 && b0 + u < total) { if (++an == a.na) { an = 0; if (++cell == gg) { cell = 0; ++b; } } }
            an_[u] = an; cell_[u] = cell;
            src[u] = a.raw + ((size_t)b * gg + cell) * a.raw_stride + an * attrs;
            rowi[u] = (size_t)b * a.rows_total + a.row_off + (size_t)cell * a.na + an;
            dst[u] = a.det + rowi[u] * attrs;
            v0[u] = lane < attrs ? src[u][lane] : 0.f;
            v1[u] = (two && lane + 64 < attrs) ? src[u][lane + 64] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (b0 + u >= total) break;
            const int an = an_[u], cell = cell_[u];
            const float r0 = lane < 4 ? yolo_box_attr(lane, v0[u], cell % a.gw, cell / a.gw, a.anchors + 2 * an, GW, GH, SX, SY, a.mode) : sigmoid_fast(v0[u]);
            const float r1 = sigmoid_fast(v1[u]);
            if (lane < attrs) dst[u][lane] = r0;
            if (two && lane + 64 < attrs) dst[u][lane + 64] = r1;
            const float obj = __shfl(r0, 4);
            float best = -INFINITY; int bi = 0x7fffffff;
            if (lane >= 5 && lane < attrs) { best = obj * r0; bi = lane - 5; }
            if (two && lane + 64 < attrs) first_max(best, bi, obj * r1, lane + 59);
            wave_argmax(best, bi);
            if (lane == 0 && scores) { scores[rowi[u]] = best; labels[rowi[u]] = bi; }
        }
    }
}

// Reductions on the vector ALU only (DPP row operations, no LDS traffic).  dpp<CTRL, ROWS>(v): v of the lane the DPP control selects, in
// the rows of ROWS (the other rows keep their own v).
template <int CTRL, int ROWS = 0xF, typename T>
__device__ __forceinline__ T dpp(T v)
{
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(i, i, CTRL, ROWS, 0xF, false));
}
// the ladder: every lane ends up with op over the 16 lanes of its DPP row
template <typename T, typename Op>
__device__ __forceinline__ T row_reduce_dpp(T v, Op op)
{
    v = op(v, dpp<0xB1>(v));       // quad_perm [1,0,3,2]
    v = op(v, dpp<0x4E>(v));       // quad_perm [2,3,0,1]
    v = op(v, dpp<0x124>(v));      // row_ror:4
    v = op(v, dpp<0x128>(v));      // row_ror:8
    return v;
}
__device__ __forceinline__ float row_max_dpp(float v) { return row_reduce_dpp(v, [](float x, float y) { return fmaxf(x, y); }); }
__device__ __forceinline__ int row_min_dpp(int v) { return row_reduce_dpp(v, [](int x, int y) { return min(x, y); }); }
// wave-wide maximum: lane 63 ends up with the maximum of all 64 lanes, which is broadcast with a readlane
__device__ __forceinline__ float wave_max_dpp(float v)
{
    v = row_max_dpp(v);
    v = fmaxf(v, dpp<0x142, 0xA>(v));      // row_bcast:15 into rows 1 and 3
    v = fmaxf(v, dpp<0x143, 0xC>(v));      // row_bcast:31 into rows 2 and 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// Ordered compaction, the step every workgroup-wide form shares: the position of this thread among the flagged threads of a 1024-thread
// workgroup (thread order), and their number.  One barrier; `wcnt` (LDS, a word per wave) may be rewritten only after a later barrier.
__device__ __forceinline__ int block_rank(bool flag, int *wcnt, int &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    int pre = 0; total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int cnt = wcnt[k]; if (k < wv) pre += cnt; total += cnt; }
    return pre + __popcll(m & ((1ull << lane) - 1ull));
}

// Same decode, one wave per grid CELL (all `na` boxes of a pixel = na*(5+C) <= 256 contiguous floats on both sides):
// lane l owns channels l, l+64, l+128, l+192, so every load and store instruction is one fully coalesced 256-B run, the
// index arithmetic is paid once per cell instead of once per box, and the per-box arg-max is a DPP max + one ballot.
// The wave-per-box form above spent ~150 instructions per box (index math, two half-empty passes, 12 bpermutes) and
// ran the 52x52 head at 2 TB/s.
template <int R>
__global__ __launch_bounds__(256) void k_decode_yolo_cell(const DecodeArgs a, float *scores, int *labels)
{
    const int attrs = 5 + a.classes, nch = a.na * attrs;
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    const int gg = a.gh * a.gw;
    const long total = (long)a.n * gg;
    const float GW = (float)a.gw, GH = (float)a.gh, SX = (float)(a.img_w / a.gw), SY = (float)(a.img_h / a.gh);
    // per-lane channel decomposition, constant over the cells
    int an_[R], k_[R]; bool ok_[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int ch = lane + 64 * r;
        ok_[r] = ch < nch;
        an_[r] = ch / attrs; k_[r] = ch - an_[r] * attrs;
    }
    bool spec_[R]; unsigned long long seen = 0; bool merged = true;      // geometry lanes; mergeable when no lane repeats
#pragma unroll
    for (int r = 0; r < R; ++r) {
        spec_[r] = ok_[r] && k_[r] < 4;
        const unsigned long long m = __ballot(spec_[r]);
        merged = merged && !(seen & m); seen |= m;
    }
    // the next cell's loads are issued before this cell is decoded (one cell of prefetch per wave: the head tensor was
    // written by the previous kernel and comes from the Infinity Cache / HBM, ~1-2 us away)
    float xn[R];
    if (wave < total) {
        const float *src = a.raw + (size_t)wave * a.raw_stride;
#pragma unroll
        for (int r = 0; r < R; ++r) xn[r] = ok_[r] ? src[lane + 64 * r] : 0.f;
    }
    for (long p = wave; p < total; p += nwaves) {
        const unsigned up = (unsigned)__builtin_amdgcn_readfirstlane((int)p);
        const int b = (int)(up / (unsigned)gg), cell = (int)(up - (unsigned)b * gg);
        const int cy = cell / a.gw, cx = cell - cy * a.gw;
        const size_t row0 = (size_t)b * a.rows_total + a.row_off + (size_t)cell * a.na;
        float *dst = a.det ? a.det + row0 * attrs : nullptr;
        float *dst4 = a.box4 ? a.box4 + row0 * 4 : nullptr;            // lean form: geometry only (the caller wants boxes, not the tensor)
        float x[R], v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) x[r] = xn[r];
        if (p + nwaves < total) {
            const float *src = a.raw + (size_t)(p + nwaves) * a.raw_stride;
#pragma unroll
            for (int r = 0; r < R; ++r) xn[r] = ok_[r] ? src[lane + 64 * r] : 0.f;
        }
        // 4 of every (5+C) channels are box geometry and need the full-precision expf; the rest take the hardware-rate
        // sigmoid.  The geometry lanes of the R registers are (normally) disjoint lane sets, so they are merged into ONE
        // register and the expensive divergent branch runs once per cell instead of once per register.
        float xs = 0.f; int ks = 4, ans = 0;
        if (merged) {
#pragma unroll
            for (int r = 0; r < R; ++r) if (spec_[r]) { xs = x[r]; ks = k_[r]; ans = an_[r]; }
            const float vs = ks < 4 ? yolo_box_attr(ks, xs, cx, cy, a.anchors + 2 * ans, GW, GH, SX, SY, a.mode) : 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                v[r] = spec_[r] ? vs : sigmoid_fast(x[r]);
                if (dst) { if (ok_[r]) dst[lane + 64 * r] = v[r]; }
                else if (spec_[r]) dst4[an_[r] * 4 + k_[r]] = v[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                v[r] = k_[r] < 4 ? yolo_box_attr(k_[r], x[r], cx, cy, a.anchors + 2 * an_[r], GW, GH, SX, SY, a.mode) : sigmoid_fast(x[r]);
                if (dst) { if (ok_[r]) dst[lane + 64 * r] = v[r]; }
                else if (spec_[r]) dst4[an_[r] * 4 + k_[r]] = v[r];
            }
        }
        if (!scores) continue;
        for (int an = 0; an < a.na; ++an) {
            // objectness of box `an` sits at channel an*attrs + 4
            const int oc = an * attrs + 4, ol = oc & 63, orr = oc >> 6;
            float ov = v[0];
#pragma unroll
            for (int r = 1; r < R; ++r) ov = orr == r ? v[r] : ov;
            const float obj = __shfl(ov, ol);
            if (obj < a.reject_below) {                  // wave-uniform: cannot pass the threshold whatever its classes say
                if (lane == 0) { scores[row0 + an] = obj; labels[row0 + an] = 0; }
                continue;
            }
            float sc[R]; float best = -INFINITY;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                sc[r] = (ok_[r] && an_[r] == an && k_[r] >= 5) ? obj * v[r] : -INFINITY;
                best = fmaxf(best, sc[r]);
            }
            best = wave_max_dpp(best);
            // first (lowest class index = lowest channel) position holding the maximum: registers in ascending order,
            // lowest lane inside a register
            int label = 0x7fffffff;
#pragma unroll
            for (int r = R - 1; r >= 0; --r) {
                const unsigned long long m = __ballot(sc[r] == best);
                if (m) label = (int)__builtin_ctzll(m) + 64 * r - an * attrs - 5;
            }
            if (lane == 0) { scores[row0 + an] = best; labels[row0 + an] = label; }
        }
    }
}

// Lean decode, objectness first, for every head of the network in one launch.  When the caller only wants boxes above a score threshold
// (yolo_detect*: no decoded tensor), a box whose objectness is below the threshold cannot pass whatever its classes say (score = objectness
// x class probability), and with trained -- or the synthetic -- weights that is 95+ % of the 10647 boxes of an image.  Phase 1: one LANE
// per box reads just the objectness logit and settles every box below the threshold with its score reported as the objectness itself,
// exactly as the cell-per-wave kernel does (which spent ~400 instructions per cell on boxes that were then thrown away: 45 us for the
// 52x52 head).  Phase 2: the boxes that remain are taken four at a time, one per 16-lane row of the wave: the row reads the box's 5 + C
// attributes as coalesced 64-byte runs (a lane-per-box loop walked 340 bytes per lane, 85 dependent-address loads each, with the other
// lanes of the wave idle), scores them, and reduces maximum and first arg-max inside the row with DPP row operations.  Same arithmetic per
// element as the cell-per-wave kernel (yolo_box_attr, sigmoid_fast), same first-maximum label: bit-identical scores, labels and boxes.
// Phase 1: one lane per box.  Boxes below the threshold are settled here; the others are appended to a list (one atomic per wave) that
// phase 2 spreads over the whole chip -- the passing boxes cluster (an anchor, an image), and a wave that had to finish its own 64
// boxes four at a time was the kernel's tail: 49 us for 14 000 boxes, 5 us without them.
__global__ __launch_bounds__(1024) void k_decode_yolo_lean_p1(const LeanArgs a, float *scores, int *labels)
{
    __shared__ int wcnt[16]; __shared__ unsigned s_base;
    const int attrs = 5 + a.classes;
    for (long base = (long)blockIdx.x * 1024; base < a.total; base += (long)gridDim.x * 1024) {      // (block-uniform trip count: barriers inside)
        const long box = base + threadIdx.x;
        const bool valid = box < a.total;
        int hd = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k) if (k < a.nheads && box >= a.h[k].box_begin) hd = k;
        // per-lane head parameters (the four heads' descriptors sit in the kernel arguments: scalar selects)
        const float *raw = a.h[0].raw, *objp = a.h[0].obj; int raw_stride = a.h[0].raw_stride, gg = a.h[0].gh * a.h[0].gw, na = a.h[0].na, row_off = a.h[0].row_off; long bb = a.h[0].box_begin;
#pragma unroll
        for (int k = 1; k < 4; ++k) if (hd == k) { raw = a.h[k].raw; objp = a.h[k].obj; raw_stride = a.h[k].raw_stride; gg = a.h[k].gh * a.h[k].gw; na = a.h[k].na; row_off = a.h[k].row_off; bb = a.h[k].box_begin; }
        const unsigned ubox = valid ? (unsigned)(box - bb) : 0u;
        const unsigned cidx = ubox / (unsigned)na; const int an = (int)(ubox - cidx * (unsigned)na);      // cell index over n * gh * gw
        const unsigned b = cidx / (unsigned)gg; const int cell = (int)(cidx - b * (unsigned)gg);
        const unsigned row = b * (unsigned)a.rows_total + (unsigned)row_off + (unsigned)cell * (unsigned)na + (unsigned)an;
        const unsigned eoff = cidx * (unsigned)raw_stride + (unsigned)(an * attrs);              // element offset of the box in its head tensor
        // (the head conv leaves the objectness logits in a compact plane as well: consecutive lanes read consecutive floats)
        const float obj = sigmoid_fast(objp ? objp[ubox] : raw[eoff + 4]);
        const bool pass = valid && !(obj < a.reject_below);
        if (valid && !pass) { scores[row] = obj; labels[row] = 0; }
        // one atomic per WORKGROUP and step (all of them hit one word: ~11 ns each, whoever issues them): wave counts through LDS
        int tot;
        const int rank = block_rank(pass, wcnt, tot);
        if (threadIdx.x == 0 && tot) s_base = atomicAdd(a.list_count, (unsigned)tot);
        __syncthreads();
        const unsigned slot = s_base + (unsigned)rank;
        // cell < 2^24 (grid <= 4096), anchor < 16, head < 4
        if (pass && slot < a.list_cap) a.list[slot] = uint4{eoff, row, (unsigned)cell | ((unsigned)an << 24) | ((unsigned)hd << 28), __float_as_uint(obj)};
    }
}
// Phase 2: one 16-lane row per listed box, grid-stride.  The row reads the box's 5 + C attributes as coalesced 64-byte runs, all loads
// issued before the first use, scores them and reduces maximum and first arg-max inside the row with DPP row operations -- the same
// arithmetic per element as the cell-per-wave kernel, the same first-maximum label: bit-identical scores, labels and boxes.
__global__ __launch_bounds__(256) void k_decode_yolo_lean_p2(const LeanArgs a, float *scores, int *labels)
{
    const int attrs = 5 + a.classes;
    const int l15 = threadIdx.x & 15;
    const unsigned rowid = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, nrows = (gridDim.x * blockDim.x) >> 4;
    unsigned count = __hip_atomic_load(a.list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (count > a.list_cap) count = a.list_cap;
    for (unsigned base = 0; base < count; base += nrows) {               // (uniform trip count: the DPP reductions want whole rows)
        const unsigned idx = base + rowid;
        const bool act = idx < count;
        const uint4 d = act ? a.list[idx] : uint4{0, 0, 0, 0};
        const unsigned r_eoff = d.x, r_row = d.y; const int r_cell = (int)(d.z & 0xffffffu), r_an = (int)((d.z >> 24) & 15u), r_hd = (int)(d.z >> 28);
        const float r_obj = __uint_as_float(d.w);
        const float *r_raw = a.h[0].raw; int r_gw = a.h[0].gw, r_gh = a.h[0].gh; float r_sx = a.h[0].sx, r_sy = a.h[0].sy;
#pragma unroll
        for (int k = 1; k < 4; ++k) if (r_hd == k) { r_raw = a.h[k].raw; r_gw = a.h[k].gw; r_gh = a.h[k].gh; r_sx = a.h[k].sx; r_sy = a.h[k].sy; }
        const float *src = r_raw + r_eoff;
        float vv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) { const int k = l15 + 16 * t; vv[t] = (act && k < attrs) ? src[k] : 0.f; }
        const float g_raw = vv[0];
        float best = -INFINITY; int label = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < 8; ++t) {                                    // ascending k inside a lane: a strict > keeps the first maximum
            const int k = l15 + 16 * t;
            if (act && k >= 5 && k < attrs) first_max(best, label, r_obj * sigmoid_fast(vv[t]), k - 5);
        }
        const float rbest = row_max_dpp(best);
        const int rlabel = row_min_dpp(best == rbest ? label : 0x7fffffff);      // lowest class index holding the maximum
        if (act && l15 < 4) {
            a.box4[(size_t)r_row * 4 + l15] = yolo_box_attr(l15, g_raw, r_cell % r_gw, r_cell / r_gw, a.h[r_hd].anchors + 2 * r_an, (float)r_gw, (float)r_gh, r_sx, r_sy, a.mode);
            if (l15 == 0) { scores[r_row] = rbest; labels[r_row] = rlabel; }
        }
    }
    // (the list counter is zeroed by the NMS kernel that follows -- PostArgs::zero_word -- or by a memset in front of phase 1 when
    //  no NMS ran since: a last-workgroup-done reset here cost a thousand more atomics on one word)
}
hipError_t launch_decode_lean(const LeanArgs &a, float *scores, int *labels, hipStream_t s)
{
    if (a.nheads < 1 || a.nheads > 4 || !a.box4 || !scores || !labels || 5 + a.classes > 128 || !a.list || !a.list_count) return hipErrorInvalidValue;
    size_t blocks = ((size_t)a.total + 1023) / 1024; if (blocks > 256 * 2) blocks = 256 * 2;
    hipLaunchKernelGGL(k_decode_yolo_lean_p1, dim3((unsigned)blocks), dim3(1024), 0, s, a, scores, labels);
    hipLaunchKernelGGL(k_decode_yolo_lean_p2, dim3(1024), dim3(256), 0, s, a, scores, labels);
    return hipGetLastError();
}

// ---- D2: V2 `decode` (V2/decode.py:13-47): sigmoid xy/obj, exp wh, softmax classes; stored as
//      (bx, by, bw, bh, obj, cls...) normalised; corners are formed at selection time ----
__global__ void k_decode_region(const DecodeArgs a)
{
    const int attrs = 5 + a.classes;
    size_t box = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int gg = a.gh * a.gw;
    const size_t total = (size_t)a.n * gg * a.na;
    if (box >= total) return;
    int an = (int)(box % a.na); size_t t = box / a.na;
    int cell = (int)(t % gg); int b = (int)(t / gg);
    const float *p = a.raw + ((size_t)b * gg + cell) * a.raw_stride + an * attrs;
    float *o = a.det + ((size_t)b * a.rows_total + a.row_off + (size_t)cell * a.na + an) * attrs;
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = region_box_attr(k, p, cell, a.gw, a.gh, a.anchors + 2 * an);
    float mx = -INFINITY;
    for (int k = 0; k < a.classes; ++k) mx = fmaxf(mx, p[5 + k]);
    float sum = 0.f;
    for (int k = 0; k < a.classes; ++k) sum += expf(p[5 + k] - mx);
    for (int k = 0; k < a.classes; ++k) o[5 + k] = expf(p[5 + k] - mx) / sum;
}

// ---- D1: YOLOv1 `_build_detector` before the selection (V1/YOLO_V1_Inference.py:213-244; darknet twin get_detection_detections
//      DN/detection_layer.c:225-254): x = (bx + col) / S, y = (by + row) / S, w = bw^2, h = bh^2 (`tf.square`, darknet's sqrt=1),
//      class-specific score = conf * cls, label = first arg-max.  98 boxes per image: one thread per box. ----
__global__ void k_decode_v1(const float *raw, int raw_stride, int n, int S, int B, int C, int sqr, float *det, int rows_total, int row_off,
                            float *scores, int *labels)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int per = S * S * B;
    if (i >= n * per) return;
    const int img = i / per, r = i - img * per, cell = r / B, b = r - cell * B;
    const float *p = raw + (size_t)img * raw_stride;
    const float *cls = p + cell * C, *box = p + S * S * (C + B) + (cell * B + b) * 4;
    const float conf = p[S * S * C + cell * B + b];
    const int attrs = 5 + C;
    const size_t row = (size_t)img * rows_total + row_off + r;
    float *o = det + row * attrs;
    o[0] = (box[0] + (float)(cell % S)) / (float)S;
    o[1] = (box[1] + (float)(cell / S)) / (float)S;
    o[2] = sqr ? box[2] * box[2] : box[2];
    o[3] = sqr ? box[3] * box[3] : box[3];
    o[4] = conf;
    float best = -INFINITY; int bi = 0;
    for (int k = 0; k < C; ++k) { const float c = cls[k]; o[5 + k] = c; const float sc = conf * c; if (sc > best) { best = sc; bi = k; } }
    if (scores) { scores[row] = best; labels[row] = bi; }
}
hipError_t launch_decode_v1(const float *raw, int raw_stride, int n, int side, int num, int classes, int sqr, float *det, int rows_total,
                            int row_off, float *scores, int *labels, hipStream_t s)
{
    const int total = n * side * side * num;
    hipLaunchKernelGGL(k_decode_v1, dim3((total + 127) / 128), dim3(128), 0, s, raw, raw_stride, n, side, num, classes, sqr, det, rows_total, row_off, scores, labels);
    return hipGetLastError();
}

hipError_t launch_decode(const DecodeArgs &a, float *scores, int *labels, hipStream_t s)
{
    if (a.gh < 1 || a.gw < 1) return hipErrorInvalidValue;
    // the lean form (no decoded tensor) of a single head exists in the cell-per-wave kernel only
    if (!a.det && (a.region || !a.box4 || !scores || a.na * (5 + a.classes) > 256 || a.raw_stride < a.na * (5 + a.classes))) return hipErrorInvalidValue;
    if (a.region) {
        size_t total = (size_t)a.n * a.gh * a.gw * a.na;
        hipLaunchKernelGGL(k_decode_region, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, s, a);
        if (scores) {
            // region heads are tiny (845 rows/image): score them with the generic row kernel
            const size_t rows = (size_t)a.gh * a.gw * a.na;
            for (int b = 0; b < a.n; ++b)
                launch_score_rows(a.det + ((size_t)b * a.rows_total + a.row_off) * (5 + a.classes), rows, 5 + a.classes,
                                  scores + (size_t)b * a.rows_total + a.row_off, labels + (size_t)b * a.rows_total + a.row_off, s);
        }
    } else {
        const int nch = a.na * (5 + a.classes);
        if (nch <= 256 && a.raw_stride >= nch) {                   // one wave per cell (every shipped topology)
            size_t cells = (size_t)a.n * a.gh * a.gw;
            size_t blocks = (cells + 3) / 4; if (blocks > 256 * 8) blocks = 256 * 8;    // persistent: 8 workgroups per CU
            if (nch <= 128) hipLaunchKernelGGL(k_decode_yolo_cell<2>, dim3((unsigned)blocks), dim3(256), 0, s, a, scores, labels);
            else hipLaunchKernelGGL(k_decode_yolo_cell<4>, dim3((unsigned)blocks), dim3(256), 0, s, a, scores, labels);
            return hipGetLastError();
        }
        size_t total = (size_t)a.n * a.gh * a.gw * a.na;           // four boxes per wave per step, grid-stride
        if (5 + a.classes > 128) return hipErrorInvalidValue;
        size_t blocks = (total + 15) / 16; if (blocks > (1u << 20)) blocks = 1u << 20;   // one step per wave: latency-bound otherwise
        hipLaunchKernelGGL(k_decode_yolo, dim3((unsigned)blocks), dim3(256), 0, s, a, scores, labels);
    }
    return hipGetLastError();
}

// ---- Frame averaging (DN/examples/demo.c remember_network + avg_predictions; RingArgs, kernels.h): ring store + mean + decode + row score of
//      one head in one launch.  One wave per (stream, cell), and nobody else touches that cell's ring entries: the wave takes the cell's
//      anchors in turn, lanes along the 5 + C attributes of a box (two passes: attrs <= 128), so the raw tensor, every ring slot and the
//      decoded rows are all read and written as contiguous runs of 5 + C floats.  Per element: the raw value is read once, its activated
//      value -- darknet's l.output: yolo_box_act / sigmoid_fast exactly as k_decode_yolo_cell forms them, region_act and the class softmax
//      as k_decode_region's -- goes to slot pos[stream], the other K - 1 slots are read (all loads issued before the first use), and
//      avg = 0; avg = avg + alpha * slot[j] for j = 0 .. K - 1 in SLOT order, uncontracted, as avg_predictions adds them.  The box formula
//      is applied to avg; objectness and classes are avg itself.  Score and label: k_score_rows' rule (first maximum of obj * class). ----
template <bool REGION>
__global__ __launch_bounds__(256) void k_decode_avg(const DecodeArgs a, const RingArgs g, float *scores, int *labels)
{
    const int attrs = 5 + a.classes, nch = a.na * attrs;
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    const int gg = a.gh * a.gw;
    const long total = (long)a.n * gg;
    const float GW = (float)a.gw, GH = (float)a.gh, SX = (float)(a.img_w / a.gw), SY = (float)(a.img_h / a.gh);
    const size_t slot = (size_t)g.max_batch * g.E;          // floats between two slots of one element
    for (long p = wave; p < total; p += nwaves) {
        const unsigned up = (unsigned)__builtin_amdgcn_readfirstlane((int)p);
        const int b = (int)(up / (unsigned)gg), cell = (int)(up - (unsigned)b * gg);
        const int cy = cell / a.gw, cx = cell - cy * a.gw;
        const int pos = g.pos[b];                           // wave-uniform, 0 .. K - 1; advanced by a later launch
        const float *src = a.raw + (size_t)up * a.raw_stride;
        float *mine = g.ring + (size_t)b * g.E + g.off + (size_t)cell * nch;      // this cell in slot 0
        const size_t row0 = (size_t)b * a.rows_total + a.row_off + (size_t)cell * a.na;
        for (int an = 0; an < a.na; ++an) {
            float x[2], old[2][8], v[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int k = lane + 64 * t;
                x[t] = k < attrs ? src[an * attrs + k] : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) old[t][j] = (j < g.K && j != pos && k < attrs) ? mine[j * slot + an * attrs + k] : 0.f;
            }
            float e[2] = {0.f, 0.f}, sum = 1.f;
            if (REGION) {                                   // softmax over the box's classes (DN/blas.c:305-321 at temperature 1)
                float mx = -INFINITY;
#pragma unroll
                for (int t = 0; t < 2; ++t) { const int k = lane + 64 * t; if (k >= 5 && k < attrs) mx = fmaxf(mx, x[t]); }
                mx = wave_max(mx);
#pragma unroll
                for (int t = 0; t < 2; ++t) { const int k = lane + 64 * t; e[t] = (k >= 5 && k < attrs) ? expf(x[t] - mx) : 0.f; }
                sum = wave_sum(e[0] + e[1]);
            }
            float *dst = a.det + (row0 + an) * attrs;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int k = lane + 64 * t;
                float act;
                if (REGION) act = k < 5 ? region_act(k, x[t]) : e[t] / sum;
                else act = k < 4 ? yolo_box_act(k, x[t]) : sigmoid_fast(x[t]);
                if (k < attrs) mine[pos * slot + an * attrs + k] = act;
                float avg = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) if (j < g.K) avg = avg + g.alpha * (j == pos ? act : old[t][j]);
                if (k >= 4) v[t] = avg;
                else if (REGION) v[t] = region_box_form(k, avg, cell, a.gw, a.gh, a.anchors + 2 * an);
                else v[t] = yolo_box_form(k, avg, cx, cy, a.anchors + 2 * an, GW, GH, SX, SY, a.mode);
                if (k < attrs) dst[k] = v[t];
            }
            const float obj = __shfl(v[0], 4);
            float best = -INFINITY; int bi = 0x7fffffff;
            if (lane >= 5 && lane < attrs) { best = obj * v[0]; bi = lane - 5; }
            if (lane + 64 < attrs) first_max(best, bi, obj * v[1], lane + 59);
            wave_argmax(best, bi);
            if (lane == 0) { scores[row0 + an] = best; labels[row0 + an] = bi; }
        }
    }
}
hipError_t launch_decode_avg(const DecodeArgs &a, const RingArgs &g, float *scores, int *labels, hipStream_t s)
{
    if (a.gh < 1 || a.gw < 1 || a.n < 1 || a.n > g.max_batch || !a.det || !scores || !labels || !g.ring || !g.pos || g.K < 2 || g.K > 8) return hipErrorInvalidValue;
    if (5 + a.classes > 128 || a.raw_stride < a.na * (5 + a.classes)) return hipErrorInvalidValue;
    const size_t cells = (size_t)a.n * a.gh * a.gw;
    size_t blocks = (cells + 3) / 4; if (blocks > 256 * 8) blocks = 256 * 8;          // as k_decode_yolo_cell: persistent, 8 workgroups per CU
    if (a.region) hipLaunchKernelGGL(k_decode_avg<true>, dim3((unsigned)blocks), dim3(256), 0, s, a, g, scores, labels);
    else hipLaunchKernelGGL(k_decode_avg<false>, dim3((unsigned)blocks), dim3(256), 0, s, a, g, scores, labels);
    return hipGetLastError();
}
__global__ void k_ring_advance(int *pos, int n, int K)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) pos[b] = (pos[b] + 1) % K;
}
hipError_t launch_ring_advance(int *pos, int n, int K, hipStream_t s)
{
    hipLaunchKernelGGL(k_ring_advance, dim3((n + 63) / 64), dim3(64), 0, s, pos, n, K);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void k_ring_slot_move(float *ring, float *keep, const int *pos, int max_batch, size_t E, int restore)
{
    const size_t total = (size_t)max_batch * E;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float *r = ring + (size_t)pos[i / E] * total + i;
        if (restore) *r = keep[i]; else keep[i] = *r;
    }
}
hipError_t launch_ring_slot_move(float *ring, float *keep, const int *pos, int max_batch, size_t E, int restore, hipStream_t s)
{
    size_t blocks = ((size_t)max_batch * E + 255) / 256; if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(k_ring_slot_move, dim3((unsigned)blocks), dim3(256), 0, s, ring, keep, pos, max_batch, E, restore);
    return hipGetLastError();
}

// ---- S: box_scores = confidence * class_prob; argmax / reduce_max (V3/YOLOV3.py:353-357).  One wave per row,
//      lanes along the attributes (coalesced), shuffle arg-max (first maximum, like argmax). ----
__global__ __launch_bounds__(256) void k_score_rows(const float *det, size_t nrows, int attrs, float *scores, int *labels, int objectness_mode)
{
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t r = wave; r < nrows; r += nwaves) {
        const float *p = det + r * attrs;
        const float obj = p[4];
        float best = -INFINITY; int bi = 0x7fffffff;
        for (int k = lane; k < attrs - 5; k += 64) {
            // objectness_mode (V3/yolo_v3.py:385,397): gate on obj alone, class = argmax of the raw class scores
            first_max(best, bi, objectness_mode ? p[5 + k] : obj * p[5 + k], k);
        }
        wave_argmax(best, bi);
        if (lane == 0) { scores[r] = objectness_mode ? obj : best; labels[r] = bi; }
    }
}
void launch_score_rows(const float *det, size_t nrows, int attrs, float *scores, int *labels, hipStream_t s, int objectness_mode)
{
    size_t blocks = (nrows + 3) / 4; if (blocks > 8192) blocks = 8192; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_score_rows, dim3((unsigned)blocks), dim3(256), 0, s, det, nrows, attrs, scores, labels, objectness_mode);
}

// TF NonMaxSuppression IOU on [y0,x0,y1,x1] rows (min/max-normalised corners, 0 when an area <= 0)
__device__ __forceinline__ float iou_tf(float4 a, float4 b)   // a,b = (x0,y0,x1,y1)
{
    float ymin_i = fminf(a.y, a.w), xmin_i = fminf(a.x, a.z), ymax_i = fmaxf(a.y, a.w), xmax_i = fmaxf(a.x, a.z);
    float ymin_j = fminf(b.y, b.w), xmin_j = fminf(b.x, b.z), ymax_j = fmaxf(b.y, b.w), xmax_j = fmaxf(b.x, b.z);
    float area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i);
    float area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j);
    if (area_i <= 0.f || area_j <= 0.f) return 0.f;
    float iy0 = fmaxf(ymin_i, ymin_j), ix0 = fmaxf(xmin_i, xmin_j);
    float iy1 = fminf(ymax_i, ymax_j), ix1 = fminf(xmax_i, xmax_j);
    float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
    return inter / ((area_i + area_j) - inter);
}
// V2/utils.py:155-174 on int32 pixel boxes: int arithmetic for the areas, float64 for the ratio
__device__ __forceinline__ double iou_v2np(int4 a, int4 b)     // (x0,y0,x1,y1) ints; the reference names them ymin.. but is symmetric
{
    int i0 = max(a.x, b.x), i1 = max(a.y, b.y), i2 = min(a.z, b.z), i3 = min(a.w, b.w);
    double ih = fmax((double)(i2 - i0), 0.), iw = fmax((double)(i3 - i1), 0.);
    double iv = ih * iw;
    int v1 = (a.z - a.x) * (a.w - a.y), v2 = (b.z - b.x) * (b.w - b.y);
    return iv / ((double)(v1 + v2) - iv);
}
// darknet box_iou (DN/box.c:152-182) on (cx,cy,w,h)
__device__ __forceinline__ float dn_overlap(float x1, float w1, float x2, float w2)
{
    float l1 = x1 - w1 / 2, l2 = x2 - w2 / 2;
    float left = l1 > l2 ? l1 : l2;
    float r1 = x1 + w1 / 2, r2 = x2 + w2 / 2;
    float right = r1 < r2 ? r1 : r2;
    return right - left;
}
__device__ __forceinline__ float iou_darknet(float4 a, float4 b)
{
    float w = dn_overlap(a.x, a.z, b.x, b.z), h = dn_overlap(a.y, a.w, b.y, b.w);
    float inter = (w < 0 || h < 0) ? 0.f : w * h;
    float uni = a.z * a.w + b.z * b.w - inter;
    return inter / uni;
}

// `_iou` of the reference's numpy NMS (V3/yolo_v3.py:350-373): float32, NO clamp of a negative overlap, +1e-05
__device__ __forceinline__ float iou_numpy_v3(float4 a, float4 b)
{
    float ix0 = fmaxf(a.x, b.x), iy0 = fmaxf(a.y, b.y), ix1 = fminf(a.z, b.z), iy1 = fminf(a.w, b.w);
    float inter = (ix1 - ix0) * (iy1 - iy0);
    float a1 = (a.z - a.x) * (a.w - a.y), a2 = (b.z - b.x) * (b.w - b.y);
    return inter / (a1 + a2 - inter + 1e-05f);
}

// correct_yolo_boxes / correct_region_boxes (DN/yolo_layer.c:247-273 = DN/region_layer.c:336-362) of attribute k (0 x, 1 y, 2 w, 3 h) of
// one box: undo the letterbox of a w x h source image (aspect-preserving size new_w x new_h) inside netw x neth; relative = 0 scales to
// source pixels.  Operation for operation darknet's (float and double mixed as there); k_darknet_boxes and the letterboxed detect path
// (cand_box) both call it, so the two round alike.
__device__ __forceinline__ float dn_correct(int k, float p, int netw, int neth, int new_w, int new_h, int w, int h, int relative)
{
    float v;
    if (k == 0) { v = (p - (netw - new_w) / 2. / netw) / ((float)new_w / netw); if (!relative) v *= w; }
    else if (k == 1) { v = (p - (neth - new_h) / 2. / neth) / ((float)new_h / neth); if (!relative) v *= h; }
    else if (k == 2) { v = p; v *= (float)netw / new_w; if (!relative) v *= w; }
    else { v = p; v *= (float)neth / new_h; if (!relative) v *= h; }
    return v;
}

// the box a candidate row enters NMS with.  A letterboxed image's row is un-letterboxed first (darknet's order: get_network_boxes, then
// do_nms_sort).  Then (cx,cy,w,h) for darknet / given corners; YOLOv1's swapped extents (see the general path below); corners
// otherwise (V3/YOLOV3.py:348-351); V2's int pixel boxes last (V2/utils.py:32-43: scale to the image, truncate to int32, clip)
__device__ __forceinline__ float4 cand_box(const PostArgs &a, int img, int row, int img_h, int img_w)
{
    const float *p = a.box4 ? a.box4 + ((size_t)img * a.rows + row) * 4 : a.det + ((size_t)img * a.rows + row) * a.attrs;
    float q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    if (a.geom && a.geom_fit == FIT_LETTERBOX) {
        const ImgDesc d = a.geom[img];
        int new_w, new_h;
        letterbox_dims(a.netw, a.neth, d.w, d.h, &new_w, &new_h);
        q0 = dn_correct(0, q0, a.netw, a.neth, new_w, new_h, d.w, d.h, a.geom_relative);
        q1 = dn_correct(1, q1, a.netw, a.neth, new_w, new_h, d.w, d.h, a.geom_relative);
        q2 = dn_correct(2, q2, a.netw, a.neth, new_w, new_h, d.w, d.h, a.geom_relative);
        q3 = dn_correct(3, q3, a.netw, a.neth, new_w, new_h, d.w, d.h, a.geom_relative);
    }
    float4 b;
    if (a.nms_mode == 2 || a.corners_in) b = float4{q0, q1, q2, q3};
    else if (a.nms_mode == 4) { float w2 = 0.5f * q2, h2 = 0.5f * q3; b = float4{q0 - h2, q1 - w2, q0 + h2, q1 + w2}; }
    else { float w2 = q2 * 0.5f, h2 = q3 * 0.5f; b = float4{q0 - w2, q1 - h2, q0 + w2, q1 + h2}; }
    if (a.nms_mode == 1 && img_w > 0) {
        int x0 = (int)(b.x * (float)img_w), y0 = (int)(b.y * (float)img_h);
        int x1 = (int)(b.z * (float)img_w), y1 = (int)(b.w * (float)img_h);
        x0 = max(x0, 0); y0 = max(y0, 0); x1 = min(x1, img_w - 1); y1 = min(y1, img_h - 1);
        b = float4{(float)x0, (float)y0, (float)x1, (float)y1};
    }
    return b;
}

#define NMS_THREADS 1024
#define SORT_LDS 4096

// LDS of k_nms_image, one pool for both paths (u64 units).  General path: sort keys [SORT_LDS] + alive bitset.  Fast path (at most
// NMS_FAST candidates, the common case: a few hundred boxes pass a detection threshold): keys, the sorted candidates themselves and the
// NMS_FAST x NMS_FAST suppression bit matrix.
#define NMS_FAST 512
#define NMS_POOL (NMS_FAST /*keys*/ + 2 * NMS_FAST /*boxes*/ + NMS_FAST / 2 * 3 /*label, score, row*/ + NMS_FAST * (NMS_FAST / 64) /*matrix*/)
static_assert(NMS_POOL >= SORT_LDS + 512, "the general path's keys + alive bitset fit the pool");

// one image's views of the workspace and of the result, and the workgroup's LDS
struct NmsImage {
    int img, img_h, img_w;
    const float *scores; const int *labels;                          // [rows]
    int *cand; unsigned long long *gkeys;                            // [rows], [rows_pow2]
    float4 *sbox; int *slabel; float *sscore; int *srow;             // sorted candidates in global memory (general paths); srow only with rows_out
    BoxOut *out; int *rows_out;                                      // [max_out]; rows_out may be null
    unsigned long long *pool; int *wave_cnt, *s_base, *s_cur, *s_kept;
    // the fast paths' carving of the pool: sorted candidates and the suppression bit matrix
    __device__ float4 *lbox() const { return (float4 *)(pool + NMS_FAST); }
    __device__ int *llabel() const { return (int *)(pool + 3 * NMS_FAST); }
    __device__ float *lscore() const { return (float *)(llabel() + NMS_FAST); }
    __device__ int *lrow() const { return llabel() + 2 * NMS_FAST; }
    __device__ unsigned long long *mat() const { return pool + 3 * NMS_FAST + NMS_FAST / 2 * 3; }
    __device__ unsigned int *alive() const { return (unsigned int *)(pool + SORT_LDS); }      // bitset for up to 32768 candidates (general paths)
};

// Sort key of candidate i (row `row`): descending score, ascending candidate index; the numpy-V3 flavour: per class (ascending), then
// objectness descending, then candidate index
__device__ __forceinline__ unsigned long long nms_key(const PostArgs &a, const NmsImage &c, int row, int i)
{
    unsigned int u = __float_as_uint(c.scores[row]);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // monotone map of float order
    if (a.nms_mode == 3) return ((unsigned long long)(c.labels[row] & 0x3ff) << 47) | ((unsigned long long)(~u) << 15) | (unsigned int)(i & 0x7fff);
    return ((unsigned long long)(~u) << 32) | (unsigned int)i;
}
// word w of the alive set before any suppression: candidates 0 .. M-1
template <typename W>
__device__ __forceinline__ W alive_init(int w, int M)
{
    constexpr int B = 8 * (int)sizeof(W);
    const int lo = w * B;
    return lo >= M ? (W)0 : (M - lo >= B) ? ~(W)0 : (W)(((W)1 << (M - lo)) - 1);
}
// does the kept candidate i remove the later candidate j (of the sorted arrays box / label)?  The three flavours of the greedy scheme:
// TF's / YOLOv1's (class-blind), darknet's and V2's numpy one (per class; V2 on int pixel boxes with a float64 ratio and the reference's
// `!(v < thr)`).  CLASS_BLIND: the caller has established that the flavour is one of the first two
template <bool CLASS_BLIND = false>
__device__ __forceinline__ bool nms_kills(const PostArgs &a, const float4 *box, const int *label, int i, int j)
{
    const float4 bi = box[i], bj = box[j];
    if (CLASS_BLIND || a.nms_mode == 0 || a.nms_mode == 4) return iou_tf(bi, bj) > a.iou_thr;
    if (a.nms_mode == 2) return label[j] == label[i] && iou_darknet(bi, bj) > a.iou_thr;
    const double v = iou_v2np(int4{(int)bi.x, (int)bi.y, (int)bi.z, (int)bi.w}, int4{(int)bj.x, (int)bj.y, (int)bj.z, (int)bj.w});
    return label[j] == label[i] && !(v < (double)a.iou_thr);
}
// record `kept` = sorted candidate i (box b) of the arrays given
__device__ __forceinline__ void nms_emit(const NmsImage &c, int kept, float4 b, const float *score, const int *label, const int *row, int i)
{
    c.out[kept] = BoxOut{b.x, b.y, b.z, b.w, score[i], label[i]};
    if (c.rows_out) c.rows_out[kept] = row[i];
}

// (1) order-preserving compaction of rows whose score passes the threshold (tf.boolean_mask order) into c.cand; returns their number.
// Every wave owns a contiguous run of rows and keeps the ballots of its 64-row steps in LDS: two barriers in all (one per 1024 rows made
// this phase a third of the kernel: a barrier of sixteen waves costs ~0.4 us)
__device__ __forceinline__ int nms_threshold_compact(const PostArgs &a, const NmsImage &c)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per_wave = ((a.rows + NMS_THREADS - 1) / NMS_THREADS) * 64;          // rows per wave, a multiple of 64 (<= 2048)
    const int steps = per_wave / 64;                                               // <= 32
    unsigned long long *const wmask = c.pool + wv * 32;                            // this wave's ballots (the pool is free until the keys are built)
    const int r_lo = wv * per_wave;
    int cnt = 0;
    // eight steps' loads in flight at a time (one load per step, each waited for by its ballot, was a chain of a dozen memory round trips)
    for (int s0 = 0; s0 < steps; s0 += 8) {
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int r = r_lo + (s0 + u) * 64 + lane; sv[u] = (s0 + u < steps && r < a.rows) ? c.scores[r] : -INFINITY; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u >= steps) break;
            const int r = r_lo + (s0 + u) * 64 + lane;
            const bool f = r < a.rows && (a.select_mode == 0 ? (sv[u] > a.score_thr) : (sv[u] >= a.score_thr));
            const unsigned long long m = __ballot(f);
            if (lane == 0) wmask[s0 + u] = m;
            cnt += __popcll(m);
        }
    }
    if (lane == 0) c.wave_cnt[wv] = cnt;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int i = 0; i < NMS_THREADS / 64; ++i) { const int n = c.wave_cnt[i]; if (i < wv) pre += n; tot += n; }
    for (int st = 0; st < steps; ++st) {
        const unsigned long long m = wmask[st];
        if ((m >> lane) & 1ull) c.cand[pre + __popcll(m & ((1ull << lane) - 1ull))] = r_lo + st * 64 + lane;
        pre += __popcll(m);
    }
    if (tid == 0) *c.s_base = tot;
    __syncthreads();
    return *c.s_base;
}

// ---- fast paths (M <= NMS_FAST): everything in LDS, five barriers (the general path pays two per kept box and ~40 for its sort).  Phase
//      times at ~150 candidates, 32 images (kernel trace, one MI355X): launch 4 us, compaction 2.5, keys + rank + gather 5, bit matrix 14,
//      scan 5.  Same keys, same gather arithmetic, same nms_kills and the same greedy order as the general path: identical records. ----
// keys, rank sort and gather of the M candidates into the LDS arrays (two barriers)
__device__ __forceinline__ void nms_sort_lds(const PostArgs &a, const NmsImage &c, int M)
{
    const int tid = threadIdx.x;
    unsigned long long *const keys = c.pool;                                                // [NMS_FAST]
    // (the compaction's last barrier also retired the ballots that shared the pool with the keys)
    if (tid < M) keys[tid] = nms_key(a, c, c.cand[tid], tid);
    __syncthreads();
    // rank sort: the keys are distinct, so a key's position is the number of smaller keys.  Eight lanes share a candidate (each
    // counts an eighth of the keys; three shuffles add the parts up), two passes of the 1024 threads cover 256 candidates
    for (int c0 = 0; c0 < M; c0 += NMS_THREADS / 8) {
        const int ci = c0 + (tid >> 3), part = tid & 7;
        const unsigned long long mykey = ci < M ? keys[ci] : 0ull;
        int rank = 0;
        for (int j = part; j < M; j += 8) rank += keys[j] < mykey ? 1 : 0;
        rank += __shfl_xor(rank, 1); rank += __shfl_xor(rank, 2); rank += __shfl_xor(rank, 4);
        if (ci < M && part == 0) {
            const int row = c.cand[ci];
            c.lbox()[rank] = cand_box(a, c.img, row, c.img_h, c.img_w); c.llabel()[rank] = c.labels[row]; c.lscore()[rank] = c.scores[row]; c.lrow()[rank] = row;
        }
    }
    __syncthreads();
}
// The flavours that stop at max_out kept boxes (TF's, YOLOv1's) need the suppression row of a KEPT box only, and kept boxes are few: one
// wave walks the candidates in order and forms the row of each box it keeps on the spot -- lane b evaluates the pair (i, 64 w + b), the
// ballot is the word -- instead of all M W words up front (14 of the kernel's 30 us for ~150 candidates, of which 20 rows were ever read)
__device__ __forceinline__ void nms_lazy(const PostArgs &a, const NmsImage &c, int M)
{
    const int lane = threadIdx.x & 63, W = (M + 63) >> 6;
    if (threadIdx.x >> 6) return;
    const float4 *const lbox = c.lbox();
    unsigned long long al = alive_init<unsigned long long>(lane, M);      // lane w holds word w of the alive set
    int kept = 0;
    for (int w = 0; w < W && kept < a.max_out; ++w) {
        while (kept < a.max_out) {
            const unsigned long long cw = __shfl(al, w);      // (wave-uniform)
            if (!cw) break;
            const int i = 64 * w + (int)__builtin_ctzll(cw);
            const float4 bc = lbox[i];
            if (lane == 0) nms_emit(c, kept, bc, c.lscore(), c.llabel(), c.lrow(), i);
            ++kept;
            for (int ww = w; ww < W; ++ww) {
                const int j = 64 * ww + lane;
                const bool kill = j > i && j < M && nms_kills<true>(a, lbox, nullptr, i, j < M ? j : i);
                unsigned long long bits = __ballot(kill);
                if (ww == w) bits |= 1ull << (i & 63);
                if (lane == ww) al &= ~bits;
            }
        }
    }
    if (lane == 0) a.counts_out[c.img] = kept;
}
// Suppression bit matrix, then a greedy scan by one wave (one barrier)
__device__ __forceinline__ void nms_matrix(const PostArgs &a, const NmsImage &c, int M)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, W = (M + 63) >> 6;
    const float4 *const lbox = c.lbox(); const int *const llabel = c.llabel();
    unsigned long long *const mat = c.mat();                                                // [M][W]
    // word (i, w) bit b set <=> candidate i, when kept, removes the later candidate j = 64 w + b.  One wave per word: lane b evaluates
    // the pair (i, 64 w + b), the ballot IS the word
    for (int e = wv; e < M * W; e += NMS_THREADS / 64) {
        const int i = e / W, w = e - i * W;
        unsigned long long bits = 0;
        if (64 * w + 63 > i) {                           // (wave-uniform)
            const int j = 64 * w + lane;
            bits = __ballot(j > i && j < M && nms_kills(a, lbox, llabel, i, j));
        }
        if (lane == 0) mat[e] = bits;
    }
    __syncthreads();
    if (wv) return;
    unsigned long long al = alive_init<unsigned long long>(lane, M);      // lane w holds word w of the alive set
    int kept = 0;
    const bool capped = a.nms_mode == 0 || a.nms_mode == 4;
    for (int w = 0; w < W; ++w) {
        while (true) {
            const unsigned long long cw = __shfl(al, w);          // (wave-uniform)
            if (!cw || (capped && kept >= a.max_out)) break;
            const int i = 64 * w + (int)__builtin_ctzll(cw);
            if (kept < a.max_out && lane == 0) nms_emit(c, kept, lbox[i], c.lscore(), llabel, c.lrow(), i);
            ++kept;
            unsigned long long kill = lane < W ? mat[i * W + lane] : 0ull;
            if (lane == w) kill |= 1ull << (i & 63);
            al &= ~kill;
        }
        if (capped && kept >= a.max_out) break;
    }
    if (lane == 0) a.counts_out[c.img] = min(kept, a.max_out);
}

// ---- general paths (any M): keys + bitonic sort in LDS (or in global memory above SORT_LDS), the sorted candidates in global memory,
//      the alive bitset in LDS.  Returns M after V2's top-400 cut. ----
__device__ __forceinline__ int nms_sort_global(const PostArgs &a, const NmsImage &c, int M)
{
    const int tid = threadIdx.x;
    int P = 1; while (P < M) P <<= 1;
    unsigned long long *const keys = P <= SORT_LDS ? c.pool : c.gkeys;
    for (int i = tid; i < P; i += NMS_THREADS) keys[i] = i < M ? nms_key(a, c, c.cand[i], i) : ~0ull;
    __syncthreads();
    // bitonic sort, ascending
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += NMS_THREADS) {
                int x = i ^ j;
                if (x > i) {
                    unsigned long long ki = keys[i], kx = keys[x];
                    bool up = (i & k) == 0;
                    if ((ki > kx) == up) { keys[i] = kx; keys[x] = ki; }
                }
            }
            __syncthreads();
        }
    if (a.nms_mode == 1 && M > 400) M = 400;           // V2 numpy flavour keeps only the 400 best before NMS (bboxes_sort top_k, V2/utils.py:146-151)
    // gather candidates in sorted order
    for (int i = tid; i < M; i += NMS_THREADS) {
        int row = c.cand[(unsigned int)(keys[i] & (a.nms_mode == 3 ? 0x7fffu : 0xffffffffu))];
        c.sbox[i] = cand_box(a, c.img, row, c.img_h, c.img_w); c.slabel[i] = c.labels[row]; c.sscore[i] = c.scores[row];
        if (c.srow) c.srow[i] = row;
    }
    for (int i = tid; i < 1024; i += NMS_THREADS) c.alive()[i] = alive_init<unsigned int>(i, M);
    if (tid == 0) { *c.s_cur = -1; *c.s_kept = 0; }
    __syncthreads();
    return M;
}
// Reference numpy NMS (V3/yolo_v3.py:376-420), class by class over the sorted list.  The reference filters `cls_scores` with indices
// taken on `cls_boxes[1:]` (:414-418), so after every round each survivor inherits the score of the element that preceded it in the
// current list -- reproduced here.
__device__ __forceinline__ void nms_numpy_v3(const PostArgs &a, const NmsImage &c, int M)
{
    const int tid = threadIdx.x;
    unsigned int *const alive = c.alive();
    __syncthreads();
    int *list = c.cand;                             // compacted alive positions (cand is free after the gather)
    float *tmp = (float *)c.gkeys;                  // scratch for the shifted scores (keys are free as well)
    __shared__ int s_seg_end;
    int seg = 0;
    while (seg < M) {
        if (tid == 0) { int e = seg + 1; const int lc = c.slabel[seg]; while (e < M && c.slabel[e] == lc) ++e; s_seg_end = e; }
        __syncthreads();
        const int seg_end = s_seg_end;
        while (true) {
            // compact the alive positions of this class segment, in order
            if (tid == 0) *c.s_base = 0;
            __syncthreads();
            for (int r0 = seg; r0 < seg_end; r0 += NMS_THREADS) {
                const int j = r0 + tid;
                const bool f = j < seg_end && ((alive[j >> 5] >> (j & 31)) & 1u);
                int tot;
                const int rank = block_rank(f, c.wave_cnt, tot);
                const int base = *c.s_base;
                if (f) list[base + rank] = j;
                __syncthreads();
                if (tid == 0) *c.s_base = base + tot;
                __syncthreads();
            }
            const int len = *c.s_base;
            if (len == 0) break;
            const int head = list[0];
            const float4 bh = c.sbox[head];
            const int kept = *c.s_kept;
            if (tid == 0) {
                if (kept < a.max_out) nms_emit(c, kept, bh, c.sscore, c.slabel, c.srow, head);
                *c.s_kept = kept + 1;
                atomicAnd(&alive[head >> 5], ~(1u << (head & 31)));
            }
            for (int m2 = 1 + tid; m2 < len; m2 += NMS_THREADS) {
                const int j = list[m2];
                if (iou_numpy_v3(bh, c.sbox[j]) < a.iou_thr) tmp[j] = c.sscore[list[m2 - 1]];     // survivor: shifted score
                else atomicAnd(&alive[j >> 5], ~(1u << (j & 31)));
            }
            __syncthreads();
            for (int m2 = 1 + tid; m2 < len; m2 += NMS_THREADS) {
                const int j = list[m2];
                if ((alive[j >> 5] >> (j & 31)) & 1u) c.sscore[j] = tmp[j];
            }
            __syncthreads();
        }
        seg = seg_end;
        __syncthreads();
    }
    if (tid == 0) a.counts_out[c.img] = min(*c.s_kept, a.max_out);
}
// greedy: the best alive candidate is kept and suppresses every later one it overlaps (two barriers per kept box)
__device__ __forceinline__ void nms_general(const PostArgs &a, const NmsImage &c, int M)
{
    const int tid = threadIdx.x;
    unsigned int *const alive = c.alive();
    int pos = 0;
    while (true) {
        if (tid == 0) {
            int cur = -1;
            for (int wd = pos >> 5; wd < ((M + 31) >> 5); ++wd) {
                unsigned int bits = alive[wd];
                if (wd == (pos >> 5)) bits &= ~((1u << (pos & 31)) - 1u);
                if (bits) { cur = wd * 32 + __ffs(bits) - 1; break; }
            }
            *c.s_cur = cur;
        }
        __syncthreads();
        const int cur = *c.s_cur, kept = *c.s_kept;
        if (cur < 0 || ((a.nms_mode == 0 || a.nms_mode == 4) && kept >= a.max_out)) break;
        if (tid == 0) {
            if (kept < a.max_out) nms_emit(c, kept, c.sbox[cur], c.sscore, c.slabel, c.srow, cur);
            *c.s_kept = kept + 1;
        }
        for (int j = cur + 1 + tid; j < M; j += NMS_THREADS) {
            if (!((alive[j >> 5] >> (j & 31)) & 1u)) continue;
            if (nms_kills(a, c.sbox, c.slabel, cur, j)) atomicAnd(&alive[j >> 5], ~(1u << (j & 31)));
        }
        pos = cur + 1;
        __syncthreads();
    }
    if (tid == 0) a.counts_out[c.img] = min(*c.s_kept, a.max_out);
}

__global__ __launch_bounds__(NMS_THREADS) void k_nms_image(const PostArgs a)
{
    __shared__ unsigned long long pool[NMS_POOL];
    __shared__ int wave_cnt[NMS_THREADS / 64];
    __shared__ int s_base, s_cur, s_kept;
    const int img = blockIdx.x, tid = threadIdx.x;
    const size_t r0 = (size_t)img * a.rows, o0 = (size_t)img * a.max_out;
    NmsImage c;
    c.img = img; c.img_h = a.img_h; c.img_w = a.img_w;
    if (a.geom && a.geom_pixels && a.nms_mode == 1) { c.img_h = a.geom[img].h; c.img_w = a.geom[img].w; }      // V2's image_shape = this image's
    c.scores = a.scores + r0; c.labels = a.labels + r0; c.cand = a.cand + r0; c.gkeys = a.keys + (size_t)img * a.rows_pow2;
    c.sbox = a.sbox + r0; c.slabel = a.slabel + r0; c.sscore = a.sscore + r0;
    c.srow = a.rows_out ? a.srow + r0 : nullptr;                       // row of every sorted candidate
    c.out = (BoxOut *)a.boxes_out + o0; c.rows_out = a.rows_out ? a.rows_out + o0 : nullptr;
    c.pool = pool; c.wave_cnt = wave_cnt; c.s_base = &s_base; c.s_cur = &s_cur; c.s_kept = &s_kept;

    // unused record slots read as zeros (this replaces a memset node in front of every launch); the kept boxes are written by thread
    // 0 after later barriers
    for (int k = tid; k < a.max_out * (int)(sizeof(BoxOut) / 4); k += NMS_THREADS) ((unsigned *)c.out)[k] = 0u;
    if (c.rows_out) for (int k = tid; k < a.max_out; k += NMS_THREADS) c.rows_out[k] = -1;
    if (a.zero_word && img == 0 && tid == 0) *a.zero_word = 0u;      // the lean decode's list counter, for the next step

    int M = nms_threshold_compact(a, c);
    if (M <= NMS_FAST && a.nms_mode != 3) {
        nms_sort_lds(a, c, M);
        if (a.nms_mode == 1 && M > 400) M = 400;           // V2 numpy flavour keeps only the 400 best before NMS (bboxes_sort top_k, V2/utils.py:146-151)
        if ((a.nms_mode == 0 || a.nms_mode == 4) && a.max_out <= 64) nms_lazy(a, c, M);
        else nms_matrix(a, c, M);
        return;
    }
    M = nms_sort_global(a, c, M);
    if (a.nms_mode == 3) nms_numpy_v3(a, c, M);
    else nms_general(a, c, M);
}

// the kept records of a stretched image, scaled to its source pixels after NMS: `convert_to_original_size` of the reference's V3 scripts,
// box * original_size for normalised boxes (V3/YOLO_V3_inference.py:55-57) and box * (original_size / size) for network-pixel boxes
// (V3/convert_ckpt_and_inference.py:43-45), both float64 in numpy: evaluated in double here and rounded once
__global__ void k_records_to_source(BoxOut *out, const int *counts, int max_out, const ImgDesc *geom, int netw, int neth, int net_pixels)
{
    const int img = blockIdx.x, k = threadIdx.x;
    const int cnt = min(counts[img], max_out);
    const ImgDesc d = geom[img];
    const double rx = net_pixels ? (double)d.w / (double)netw : (double)d.w, ry = net_pixels ? (double)d.h / (double)neth : (double)d.h;
    for (int r = k; r < cnt; r += blockDim.x) {
        BoxOut &b = out[(size_t)img * max_out + r];
        b.x0 = (float)((double)b.x0 * rx); b.y0 = (float)((double)b.y0 * ry);
        b.x1 = (float)((double)b.x1 * rx); b.y1 = (float)((double)b.y1 * ry);
    }
}

hipError_t launch_postprocess(const PostArgs &a, hipStream_t s)
{
    size_t nrows = (size_t)a.n * a.rows;
    if (!a.scores_ready) launch_score_rows(a.det, nrows, a.attrs, a.scores, a.labels, s, a.nms_mode == 3);
    hipLaunchKernelGGL(k_nms_image, dim3(a.n), dim3(NMS_THREADS), 0, s, a);
    if (a.geom && a.geom_pixels && a.geom_fit != FIT_LETTERBOX && a.nms_mode != 1)
        hipLaunchKernelGGL(k_records_to_source, dim3(a.n), dim3(64), 0, s, (BoxOut *)a.boxes_out, (const int *)a.counts_out, a.max_out, a.geom, a.netw, a.neth, a.geom_net_pixels);
    return hipGetLastError();
}

// ---- cross-window merge of yolo_detect_tiled_u8 (TileMergeArgs, kernels.h; DESIGN.md "Tiled detection") ----
// The box row `p` = (cx, cy, w, h) of a window enters its image's merged list with: in source-image pixels.  A DECODE_PIXEL head's numbers are
// divided by the network size first.  STRETCH: the box in window units times the window's extent, plus the window's origin.  LETTERBOX:
// correct_yolo_boxes for the window with relative = 0 (dn_correct, as cand_box applies it per image), plus the origin.  Corners are formed
// from (cx, cy, w, h) in window units by cand_box's arithmetic (q - w * 0.5, q + w * 0.5) before the origin is added.  Every step is one
// unfused fp32 operation (dn_correct: darknet's own mix of float and double), so a numpy float32 restatement reproduces it bit for bit.
__device__ __forceinline__ float4 tile_box(const TileMergeArgs &a, const WinDesc &w, const float *p)
{
    float q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    if (a.net_pixels) { q0 = __fdiv_rn(q0, (float)a.netw); q1 = __fdiv_rn(q1, (float)a.neth); q2 = __fdiv_rn(q2, (float)a.netw); q3 = __fdiv_rn(q3, (float)a.neth); }
    float sx = (float)w.w, sy = (float)w.h;          // what a window unit is in pixels
    if (a.fit == FIT_LETTERBOX) {
        int new_w, new_h;
        letterbox_dims(a.netw, a.neth, w.w, w.h, &new_w, &new_h);
        q0 = dn_correct(0, q0, a.netw, a.neth, new_w, new_h, w.w, w.h, 0); q1 = dn_correct(1, q1, a.netw, a.neth, new_w, new_h, w.w, w.h, 0);
        q2 = dn_correct(2, q2, a.netw, a.neth, new_w, new_h, w.w, w.h, 0); q3 = dn_correct(3, q3, a.netw, a.neth, new_w, new_h, w.w, w.h, 0);
        sx = sy = 1.f;                                // already pixels of the window (a product with 1 is exact)
    }
    const float X = (float)w.x0, Y = (float)w.y0;
    if (a.centre) return float4{__fadd_rn(__fmul_rn(q0, sx), X), __fadd_rn(__fmul_rn(q1, sy), Y), __fmul_rn(q2, sx), __fmul_rn(q3, sy)};
    const float w2 = __fmul_rn(q2, 0.5f), h2 = __fmul_rn(q3, 0.5f);
    return float4{__fadd_rn(__fmul_rn(__fsub_rn(q0, w2), sx), X), __fadd_rn(__fmul_rn(__fsub_rn(q1, h2), sy), Y),
                  __fadd_rn(__fmul_rn(__fadd_rn(q0, w2), sx), X), __fadd_rn(__fmul_rn(__fadd_rn(q1, h2), sy), Y)};
}
__device__ __forceinline__ bool tile_pass(const TileMergeArgs &a, float score) { return a.select_mode == 0 ? score > a.score_thr : score >= a.score_thr; }

// launch 1: one workgroup per window of the step counts its passing rows
__global__ __launch_bounds__(1024) void k_tile_count(const TileMergeArgs a)
{
    __shared__ int wcnt[16];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *sc = a.scores + (size_t)b * a.rows;
    int cnt = 0;
    for (int r = threadIdx.x; r < a.rows; r += 1024) cnt += tile_pass(a, sc[r]) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) wcnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += wcnt[k]; a.wcount[b] = t; }
}
// launch 2: one workgroup per window of the step writes its passing rows, in row order, at its place in the image's list
__global__ __launch_bounds__(1024) void k_tile_write(const TileMergeArgs a)
{
    __shared__ int wcnt[16]; __shared__ int s_before;
    const int b = blockIdx.x, wi = a.first + b, tid = threadIdx.x;
    const WinDesc w = a.wins[wi];
    const int image = w.image;
    // rows of this image ahead of the window: what earlier steps merged -- only where the image's windows began in an earlier step, i.e. the
    // step's first window continues it -- plus the image's earlier windows of this step
    if (tid == 0) s_before = (a.first > 0 && a.wins[a.first].image == image && a.wins[a.first - 1].image == image) ? a.run_in[image] : 0;
    __syncthreads();
    for (int t = tid; t < b; t += 1024) if (a.wins[a.first + t].image == image) atomicAdd(&s_before, a.wcount[t]);      // (integer sum: any order, one value)
    __syncthreads();
    int pos = s_before;
    const int mine = a.wcount[b];
    const size_t s0 = (size_t)b * a.rows, m0 = (size_t)image * a.cap;
    for (int r0 = 0; r0 < a.rows; r0 += 1024) {          // (uniform trip count: barriers inside)
        const int r = r0 + tid;
        const bool f = r < a.rows && tile_pass(a, a.scores[s0 + r]);
        int tot;
        const int at = pos + block_rank(f, wcnt, tot);
        if (f && at < a.cap) {
            a.m_scores[m0 + at] = a.scores[s0 + r]; a.m_labels[m0 + at] = a.labels[s0 + r];
            a.m_box[m0 + at] = tile_box(a, w, a.box4 ? a.box4 + (s0 + r) * 4 : a.det + (s0 + r) * a.attrs);
        }
        pos += tot;
        __syncthreads();          // wcnt is rewritten by the next round
    }
    if (tid != 0) return;
    const int after = s_before + mine;
    const bool last_of_step = b == a.nb - 1 || a.wins[wi + 1].image != image, last_of_image = wi == a.nwin - 1 || a.wins[wi + 1].image != image;
    if (last_of_step) a.run_out[image] = after;
    if (last_of_image) {
        a.total[image] = after;
        if (after > a.cap) atomicMin(a.overflow, ((unsigned long long)(unsigned)image << 32) | (unsigned)after);
    }
}
hipError_t launch_tile_merge(const TileMergeArgs &a, hipStream_t s)
{
    if (a.nb < 1 || a.first < 0 || a.first + a.nb > a.nwin || a.rows < 1 || a.cap < 1 || a.cap > TILE_MERGE_CAP || (a.fit != FIT_STRETCH && a.fit != FIT_LETTERBOX)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tile_count, dim3(a.nb), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_tile_write, dim3(a.nb), dim3(1024), 0, s, a);
    return hipGetLastError();
}
__global__ void k_tile_relative(BoxOut *out, const int *counts, int max_out, const ImgDesc *descs)
{
    const int img = blockIdx.x;
    const int cnt = min(counts[img], max_out);
    const float W = (float)descs[img].w, H = (float)descs[img].h;
    for (int r = threadIdx.x; r < cnt; r += blockDim.x) {
        BoxOut &b = out[(size_t)img * max_out + r];
        b.x0 = __fdiv_rn(b.x0, W); b.y0 = __fdiv_rn(b.y0, H); b.x1 = __fdiv_rn(b.x1, W); b.y1 = __fdiv_rn(b.y1, H);
    }
}
hipError_t launch_tile_relative(void *boxes, const int *counts, int max_out, const ImgDesc *descs, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_tile_relative, dim3(n), dim3(64), 0, s, (BoxOut *)boxes, counts, max_out, descs);
    return hipGetLastError();
}

// ---- X: `detections_boxes` (V3/yolo_v3.py:329-347): (cx, cy, w, h, rest...) -> (x0, y0, x1, y1, rest...), w/2 form ----
__global__ void k_boxes_to_corners(const float *in, float *out, size_t nrows, int attrs)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * attrs) return;
    size_t r = idx / attrs; int k = (int)(idx - r * attrs);
    const float *p = in + r * attrs;
    float v;
    if (k == 0) v = p[0] - p[2] / 2.0f;
    else if (k == 1) v = p[1] - p[3] / 2.0f;
    else if (k == 2) v = p[0] + p[2] / 2.0f;
    else if (k == 3) v = p[1] + p[3] / 2.0f;
    else v = p[k];
    out[idx] = v;
}
hipError_t launch_boxes_to_corners(const float *in, float *out, size_t nrows, int attrs, hipStream_t s)
{
    size_t total = nrows * attrs;
    hipLaunchKernelGGL(k_boxes_to_corners, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, nrows, attrs);
    return hipGetLastError();
}

// ---- darknet do_nms_sort / do_nms_obj (DN/box.c:21-89) on caller-shaped arrays: boxes [n] (cx,cy,w,h), prob [n][classes],
//      objectness [n]; suppressed entries are zeroed in place.  One workgroup per class (sort) or one in all (obj):
//      bitonic sort of (score, index) keys in LDS (descending; ties: lower index first -- qsort leaves tie order
//      unspecified), then the reference's greedy pass with the inner loop spread over the threads.  Detections with
//      objectness == 0 do not take part (the reference moves them behind `total`). ----
#define NMSD_MAX 4096
__global__ __launch_bounds__(1024) void k_nms_dets(const float4 *boxes, float *prob, float *objectness, int n, int classes, float thresh, int by_obj)
{
    __shared__ unsigned long long key[NMSD_MAX];
    __shared__ unsigned char dead[NMSD_MAX];
    const int k = by_obj ? -1 : (int)blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    int np2 = 1; while (np2 < n) np2 <<= 1;
    for (int j = tid; j < np2; j += nt) {
        float sc = 0.f;
        if (j < n && objectness[j] != 0.f) sc = by_obj ? objectness[j] : prob[(size_t)j * classes + k];
        // descending order == ascending order of the complemented key; zero / padded entries sort last
        const unsigned bits = sc > 0.f ? __float_as_uint(sc) : 0u;
        key[j] = ((unsigned long long)(~bits) << 32) | (unsigned)j;
        dead[j] = !(j < n && objectness[j] != 0.f);
    }
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < np2 / 2; t += nt) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = key[lo], b = key[hi];
                if ((a > b) == up) { key[lo] = b; key[hi] = a; }
            }
            __syncthreads();
        }
    // greedy pass over the sorted order (every condition below is uniform across the workgroup: it only reads shared /
    // global state that was last written before a barrier).  `dead` is indexed by ORIGINAL detection index.
    for (int i = 0; i < n; ++i) {
        const unsigned ji = (unsigned)(key[i] & 0xffffffffu);
        if (ji >= (unsigned)n) break;                                   // only padding from here on
        const float si = dead[ji] ? 0.f : (by_obj ? objectness[ji] : prob[(size_t)ji * classes + k]);
        if (si != 0.f) {
            const float4 a = boxes[ji];
            for (int jj = i + 1 + tid; jj < n; jj += nt) {
                const unsigned j = (unsigned)(key[jj] & 0xffffffffu);
                if (j >= (unsigned)n || dead[j]) continue;
                if (by_obj && objectness[j] == 0.f) continue;
                if (iou_darknet(a, boxes[j]) > thresh) {
                    if (by_obj) { objectness[j] = 0.f; for (int c = 0; c < classes; ++c) prob[(size_t)j * classes + c] = 0.f; }
                    else prob[(size_t)j * classes + k] = 0.f;
                }
            }
        }
        __syncthreads();
    }
}
hipError_t launch_nms_dets(const float4 *boxes, float *prob, float *objectness, int n, int classes, float thresh, int by_obj, hipStream_t s)
{
    if (n < 1) return hipSuccess;
    if (n > NMSD_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_nms_dets, dim3(by_obj ? 1 : classes), dim3(1024), 0, s, boxes, prob, objectness, n, classes, thresh, by_obj);
    return hipGetLastError();
}

// ---- darknet's get_network_boxes on the device (DN/network.c:536-567): num_detections + fill_network_boxes over the decoded rows
//      of one image.  [yolo] heads (get_yolo_detections, DN/yolo_layer.c:316-343): rows with objectness > thresh, in head / cell /
//      anchor order, prob[j] = objectness * class_j gated by thresh.  [region] heads without a tree (get_region_detections,
//      DN/region_layer.c:364-437): every box, anchor-major, objectness and probabilities gated by thresh.  Then
//      correct_yolo_boxes / correct_region_boxes (DN/yolo_layer.c:247-273 = DN/region_layer.c:336-362: undo the letterbox).  The
//      box arithmetic below restates those lines operation for operation (the reference mixes float and double there, and the
//      veneer is compared with it to the last bits) -- this file is built with -ffp-contract=off.
//      One workgroup: an ordered compaction of ~10^4 rows is latency-, not bandwidth-bound. ----
__global__ __launch_bounds__(1024) void k_darknet_boxes(const DnBoxesArgs a)
{
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int hd = 0; hd < a.nheads; ++hd) {
        const int cells = a.cells[hd], rows = cells * a.na[hd];
        if (a.kind[hd] == 2) {
            // [detection]: no selection, no reordering -- box i * num + n of the layer is record i * num + n
            const int base = s_base;
            for (int r = tid; r < rows; r += 1024) if (base + r < a.cap) a.src[base + r] = a.off[hd] + r;
            __syncthreads();
            if (tid == 0) s_base = base + rows;
            __syncthreads();
        } else if (a.kind[hd] == 1) {
            const int base = s_base;
            for (int r = tid; r < rows; r += 1024) {
                const int i = r / a.na[hd], n = r - i * a.na[hd];
                const int pos = base + n * cells + i;              // index = n * w * h + i (DN/region_layer.c:395)
                if (pos < a.cap) a.src[pos] = a.off[hd] + r;
            }
            __syncthreads();
            if (tid == 0) s_base = base + rows;
            __syncthreads();
        } else {
            for (int r0 = 0; r0 < rows; r0 += 1024) {
                const int r = r0 + tid;
                const bool keep = r < rows && a.det[(size_t)(a.off[hd] + r) * a.attrs + 4] > a.thresh;
                int total;
                const int rank = block_rank(keep, s_wave, total), pos = s_base + rank;
                if (keep && pos < a.cap) a.src[pos] = a.off[hd] + r;
                __syncthreads();
                if (tid == 0) s_base += total;
                __syncthreads();
            }
        }
    }
    const int count = s_base;
    if (tid == 0) *a.count = count;
    if (!a.rec) return;
    __threadfence_block();
    const int n = count < a.cap ? count : a.cap;
    const int netw = a.netw, neth = a.neth, w = a.w, h = a.h;
    int new_w, new_h;
    letterbox_dims(netw, neth, w, h, &new_w, &new_h);
    // which head a row belongs to decides the gating
    for (long idx = tid; idx < (long)n * a.attrs; idx += 1024) {
        const int rec = (int)(idx / a.attrs), k = (int)(idx - (long)rec * a.attrs);
        const int row = a.src[rec];
        int kind = 0;
        for (int hd = 0; hd < a.nheads; ++hd) if (row >= a.off[hd]) kind = a.kind[hd];
        if (kind == 2) {
            // operation for operation get_detection_detections: (pred + col) / side * w in float, pow(pred, 2) * w through double
            const int hd0 = 0, r = row - a.off[hd0], nb = a.na[hd0], i = r / nb, n = r - i * nb, side = a.side;
            const float *pr = a.raw;
            const float scale = pr[side * side * a.classes + i * nb + n];
            const float *bx = pr + side * side * (a.classes + nb) + (i * nb + n) * 4;
            float v;
            if (k == 0) v = (bx[0] + (i % side)) / side * w;
            else if (k == 1) v = (bx[1] + (i / side)) / side * h;
            else if (k == 2) v = (float)(pow((double)bx[2], a.sqr ? 2 : 1) * w);
            else if (k == 3) v = (float)(pow((double)bx[3], a.sqr ? 2 : 1) * h);
            else if (k == 4) v = scale;
            else { const float prob = scale * pr[i * a.classes + (k - 5)]; v = prob > a.thresh ? prob : 0.f; }
            a.rec[idx] = v;
            continue;
        }
        const float *p = a.det + (size_t)row * a.attrs;
        const float obj_raw = p[4];
        const float objectness = kind == 1 ? (obj_raw > a.thresh ? obj_raw : 0.f) : obj_raw;
        float v;
        if (k < 4) v = dn_correct(k, p[k], netw, neth, new_w, new_h, w, h, a.relative);
        else if (k == 4) v = objectness;
        else { const float prob = obj_raw * p[k]; v = (objectness != 0.f && prob > a.thresh) ? prob : 0.f; }
        a.rec[idx] = v;
    }
}
hipError_t launch_darknet_boxes(const DnBoxesArgs &a, hipStream_t s)
{
    if (a.nheads < 1 || a.nheads > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_darknet_boxes, dim3(1), dim3(1024), 0, s, a);
    return hipGetLastError();
}

// ---- the last layer's output in darknet's own layout, what `network_predict` returns (DN/network.c:497-508 -> net->output):
//      a [yolo] layer's output is its input with the logistic applied to x, y, objectness and the class scores
//      (DN/yolo_layer.c:143-152), a [region] layer's (softmax form) the logistic on x, y, objectness and a softmax over the classes
//      (DN/region_layer.c:163-200), both planar [anchor * (5 + classes) + attr][cell].  logistic = 1./(1. + exp(-x)) evaluated in
//      double like DN/activations.h:38. ----
__global__ void k_head_darknet_layout(const float *raw, int raw_stride, int cells, int na, int classes, int region, float *out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= cells * na) return;
    const int cell = r / na, n = r - cell * na, attrs = 5 + classes;
    const float *p = raw + (size_t)cell * raw_stride + n * attrs;
    float *o = out + (size_t)n * attrs * cells + cell;
#pragma unroll
    for (int k = 0; k < 5; ++k) o[(size_t)k * cells] = darknet_layout_box_attr(k, p);
    if (!region) {
        for (int k = 0; k < classes; ++k) o[(size_t)(5 + k) * cells] = darknet_layout_box_attr(0, p + 5 + k);
    } else {
        // softmax (DN/blas.c:305-321, temperature 1): largest first, exp(x - largest), normalised by the running sum
        float largest = -3.402823466e+38f;
        for (int k = 0; k < classes; ++k) if (p[5 + k] > largest) largest = p[5 + k];
        float sum = 0.f;
        for (int k = 0; k < classes; ++k) { const float e = (float)exp((double)(p[5 + k] - largest)); sum += e; o[(size_t)(5 + k) * cells] = e; }
        for (int k = 0; k < classes; ++k) o[(size_t)(5 + k) * cells] /= sum;
    }
}
hipError_t launch_head_darknet_layout(const float *raw, int raw_stride, int cells, int na, int classes, int region, float *out, hipStream_t s)
{
    const int rows = cells * na;
    hipLaunchKernelGGL(k_head_darknet_layout, dim3((rows + 255) / 256), dim3(256), 0, s, raw, raw_stride, cells, na, classes, region, out);
    return hipGetLastError();
}
