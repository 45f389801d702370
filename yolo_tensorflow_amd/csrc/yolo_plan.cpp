// Planner of libyolo_hip.so: darknet cfg text -> layers, fusions, buffer pool (see yolo_ctx.h for the map of the host side).
//
// What the reference does with a Python graph builder + tf.Session (V3/yolo_v3.py:195-267,
// D2T/YOLO_V3_convert_darkenet_to_Tensorflow.py:435-545) or with parse_network_cfg + forward_network
// (DN/parser.c:730-875, DN/network.c:188-211) is done here once at yolo_create(), by build_plan(): a sequence of file-static steps, each
// with a header that says what it reads from the steps before it and what it writes.  In order:
//   1. parse_sections: [net], then one parser per section kind (section_table) over a cursor of the running geometry; after each layer
//      inherit_form gives a layer that moves data the type and pair form of what it moves.  Shapes, types, padded sizes, totals;
//   2. heads_to_fp32, classifier_tail, network_kind (detector / classifier / map), input_norm_and_row_limit;
//   3. count_uses, fold_shortcuts: `shortcut` after a conv is folded into that conv's epilogue (V3/yolo_v3.py:54-60);
//   4. the marking passes -- mark_resblocks, mark_stem, mark_pair_stem, mark_halo_and_s2, mark_c3s2, mark_tails -- which choose a conv's
//      own kernel, the fused launch it is a member of and the 1x1 conv that rides in its epilogue.  Their order matters: the comment in
//      build_plan() says why;
//   5. storage: decide_inplace; place_route_sources (route/concat is never executed: producers write straight into a channel window of the
//      concat buffer -- DN/route_layer.c:74-89 and tf.concat V3/yolo_v3.py:247,259 become strides); create_storages;
//      redirect_folded_convs; compute_liveness; assign_pool (liveness-based reuse of a small pool of HBM buffers, so consecutive layers
//      recycle the same few allocations and stay in L2 / Infinity Cache).
// allocate() then turns the pool into device memory.  Batch-norm is folded into the filters at weight-load time (yolo_pack.cpp).
// The planner needs no device: yolo_plan_check / yolo_plan_table / yolo_plan_dump at the end of this file run it alone, and
// tests/test_plan_table.py and tests/test_plan_dump.py pin what it writes.
#include "yolo_ctx.h"

namespace yolo_impl {

// ---- cfg parsing (DN/parser.c:730-875 read_cfg + option_find_*) ------------------------------
bool parse_cfg(const char *text, std::vector<Section> &out, std::string &err)
{
    std::string s(text ? text : "");
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t e = s.find('\n', pos); if (e == std::string::npos) e = s.size();
        std::string line = s.substr(pos, e - pos); pos = e + 1;
        size_t a = line.find_first_not_of(" \t\r"); if (a == std::string::npos) continue;
        size_t b = line.find_last_not_of(" \t\r"); line = line.substr(a, b - a + 1);
        if (line[0] == '#' || line[0] == ';') continue;
        if (line[0] == '[') {
            size_t r = line.find(']'); if (r == std::string::npos) { err = "cfg: unterminated section " + line; return false; }
            Section sec; sec.type = line.substr(1, r - 1); out.push_back(sec);
        } else {
            size_t eq = line.find('='); if (eq == std::string::npos || out.empty()) { err = "cfg: bad line '" + line + "'"; return false; }
            std::string k = line.substr(0, eq), v = line.substr(eq + 1);
            auto trim = [](std::string &t) { size_t x = t.find_first_not_of(" \t"); size_t y = t.find_last_not_of(" \t"); t = x == std::string::npos ? "" : t.substr(x, y - x + 1); };
            trim(k); trim(v); out.back().kv[k] = v;
        }
    }
    if (out.empty() || (out[0].type != "net" && out[0].type != "network")) { err = "cfg: first section must be [net]"; return false; }
    return true;
}
int opt_i(const Section &s, const char *k, int d) { auto it = s.kv.find(k); return it == s.kv.end() ? d : atoi(it->second.c_str()); }
std::string opt_s(const Section &s, const char *k, const char *d) { auto it = s.kv.find(k); return it == s.kv.end() ? std::string(d) : it->second; }
std::vector<float> opt_list(const Section &s, const char *k)
{
    std::vector<float> v; auto it = s.kv.find(k); if (it == s.kv.end()) return v;
    const char *p = it->second.c_str();
    while (*p) { char *e; double d = strtod(p, &e); if (e == p) break; v.push_back((float)d); p = e; while (*p == ',' || *p == ' ') ++p; }
    return v;
}

// The descent form of a tree head is the default of yolo_detect* only once it is measured as not slower than the full form on the
// YOLO9000 shape (tools/tree_decode_rate.py); until then the full form is
#define TREE_DESCENT_DEFAULT 0

// tree= of layer i: read and checked (yolo_tree.cpp), its size against the `want` values the layer has
static int plan_tree(yolo_ctx *c, int i, const char *section, const std::string &path, int want, const char *of)
{
    Tree t; std::string err;
    if (int r = load_tree(path, t, err)) return fail(c, r, "layer %d: [%s] %s", i, section, err.c_str());
    if (t.n != want) return fail(c, YOLO_ERR_INVALID, "layer %d: [%s] tree '%s' has %d nodes but the layer has %d %s", i, section, path.c_str(), t.n, want, of);
    c->trees.push_back(std::move(t)); c->layers[i].tree = (int)c->trees.size() - 1;
    return YOLO_OK;
}

// activation= of layer i (DN/parser.c: `logistic` where a [convolutional] / [connected] / [local] section names none, `linear` for a
// [shortcut]), the ONE place a name becomes a code.  A [shortcut] keeps any of them in L.act (k_shortcut applies it).  The other layers keep
// a slope-family activation in L.act, their kernel's own epilogue; any other one leaves the epilogue linear and becomes L.post_act, applied
// in place on the layer's output by k_activate.
static int plan_activation(yolo_ctx *c, int i, const Section &s, const char *dflt, bool shortcut)
{
    Layer &L = c->layers[i];
    const std::string name = opt_s(s, "activation", dflt);
    const int code = act_from_name(name.c_str());
    if (code < 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: activation '%s' unsupported", i, name.c_str());
    if (shortcut || act_is_slope(code)) { L.act = code; return YOLO_OK; }
    if (c->dtype == YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: activation '%s' is not served in the fp8 configuration", i, name.c_str());
    L.act = ACT_LINEAR; L.post_act = code;
    return YOLO_OK;
}

TView view_of(const yolo_ctx *c, int idx) { return idx < 0 ? c->input : c->layers[idx].out; }

// ---- section parsing: one function per section kind, found by name in section_table -----------------------------------------
// Every parser reads: the cursor (what layer i receives), the layers in front of i.  Writes: its own Layer's keys, in_dt / store_dt / pair where
// the layer computes, the cursor (what it produces), c->rows / attrs / conv_flops / weights_count / trees / tree_head, `head` on its producer.

// the running geometry while the sections are read: on entry what layer i receives, on return what it produces
struct Cursor {
    yolo_ctx *c; int i, H, W, C;
    void dims(int idx, int &h, int &w, int &ch) const { if (idx < 0) { h = c->in_h; w = c->in_w; ch = c->in_c; } else { h = c->layers[idx].H; w = c->layers[idx].W; ch = c->layers[idx].C; } }
};

// the keys the three convolution kinds share (DN/parser.c: pad=1 means size / 2, else padding= is taken literally)
static void read_conv_keys(const Section &s, Layer &L)
{
    L.filters = opt_i(s, "filters", 1); L.size = opt_i(s, "size", 1); L.stride = opt_i(s, "stride", 1);
    L.pad = opt_i(s, "pad", 0) ? L.size / 2 : opt_i(s, "padding", 0);
    L.bn = opt_i(s, "batch_normalize", 0);
}
// ... their output geometry, (H + 2p - k) / s + 1, and what they add to the context's totals: `cin_g` input channels per filter over an h x w grid
static void conv_out(Cursor &k, const Layer &L) { k.H = (k.H + 2 * L.pad - L.size) / L.stride + 1; k.W = (k.W + 2 * L.pad - L.size) / L.stride + 1; k.C = L.filters; }
static void conv_totals(yolo_ctx *c, const Layer &L, int cin_g, int h, int w)
{
    c->conv_flops += 2.0 * L.size * L.size * cin_g * L.filters * (double)h * w;
    c->weights_count += (size_t)L.filters * (L.bn ? 4 : 1) + (size_t)L.filters * cin_g * L.size * L.size;
}

// ---- the side convs (is_side_conv): layer kinds of their own with their own kernels, never a member of a fused launch, neither end of a 1x1 tail,
// no host of a folded [shortcut] and nothing for the tile tuner to choose -- every marking pass asks for L_CONV.  Size, stride and padding limits
// are each kind's own; what they plan alike is here
static std::string side_conv_name(const Layer &L)      // as the messages name the kind
{
    return L.type == L_DECONV ? "[deconvolutional]" : L.type == L_GCONV ? "[convolutional] with groups=" + std::to_string(L.groups) : "[convolutional] with xnor=1";
}
static int side_conv_dtype(yolo_ctx *c, int i, const Layer &L)
{
    if (c->dtype == YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: %s is not served in the fp8 configuration", i, side_conv_name(L).c_str());
    if (c->split()) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: %s is not served in the split-fp16 configuration", i, side_conv_name(L).c_str());
    return YOLO_OK;
}
// activation, operand and storage type, channels, the filter layout's kpad / cout_pad (cout_pad * kpad elements of filters; an xnor conv: bytes)
static int side_conv_tail(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c;
    if (int r = plan_activation(c, k.i, s, "logistic", false)) return r;
    L.in_dt = c->act_dt(); L.store_dt = c->act_dt();
    L.cin = k.C; L.cin_pad = roundup(k.C, 8);
    side_layout(L, L.kpad, L.cout_pad);
    return YOLO_OK;
}
// a grouped or xnor conv as the layer in front of head i (a [deconvolutional] there gets the head's own "must follow" message)
static int side_conv_before_head(yolo_ctx *c, int i, const char *head, const char *why_grouped, const char *why_xnor)
{
    if (i == 0 || !is_side_conv(c->layers[i - 1]) || c->layers[i - 1].type == L_DECONV) return YOLO_OK;
    const Layer &P = c->layers[i - 1];
    return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: a %s directly in front of a [%s] head is not served (%s)", i - 1, side_conv_name(P).c_str(), head, P.type == L_XCONV ? why_xnor : why_grouped);
}

// grouped convolution (DN/parser.c:184, DN/convolutional_layer.c:458-471), gconv.hip
static int parse_grouped_conv(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_GCONV; L.groups = opt_i(s, "groups", 1);
    if (L.groups < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [convolutional] groups=%d", i, L.groups);
    if (int r = side_conv_dtype(c, i, L)) return r;
    if (i == 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [convolutional] with groups=%d as the network's first layer is not served (the image is read by the dense kernels only)", i, L.groups);
    read_conv_keys(s, L);
    if (L.filters < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: conv filters %d", i, L.filters);
    if (k.C % L.groups) return fail(c, YOLO_ERR_INVALID, "layer %d: groups=%d does not divide the %d input channels", i, L.groups, k.C);
    if (L.filters % L.groups) return fail(c, YOLO_ERR_INVALID, "layer %d: groups=%d does not divide filters=%d", i, L.groups, L.filters);
    if (L.size < 1 || L.size > GCONV_MAX_SIZE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: grouped conv size %d (1..%d are served)", i, L.size, GCONV_MAX_SIZE);
    if (L.stride < 1 || L.stride > GCONV_MAX_STRIDE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: grouped conv stride %d (1..%d are served)", i, L.stride, GCONV_MAX_STRIDE);
    if (L.pad < 0 || L.pad >= L.size) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: grouped conv padding %d must be below its size %d", i, L.pad, L.size);
    if (k.H + 2 * L.pad < L.size || k.W + 2 * L.pad < L.size) return fail(c, YOLO_ERR_INVALID, "layer %d: grouped conv larger than its padded input", i);
    if (int r = side_conv_tail(k, s, L)) return r;
    conv_out(k, L);
    conv_totals(c, L, L.cin / L.groups, k.H, k.W);      // DN/convolutional_layer.c:201, :325: c / groups
    return YOLO_OK;
}

// XNOR convolution (xnor=1, DN/parser.c:198, DN/convolutional_layer.c:451-456), xconv.hip: the sum of signs on the int8 MFMA.  (binary=1 without
// xnor, and flipped=1, are read by nobody: DESIGN.md 7)
static int parse_xnor_conv(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_XCONV;
    if (opt_i(s, "groups", 1) != 1) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [convolutional] with xnor=1 and groups=%d is not served (a grouped XNOR conv)", i, opt_i(s, "groups", 1));
    if (int r = side_conv_dtype(c, i, L)) return r;
    if (i == 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [convolutional] with xnor=1 as the network's first layer is not served (the image is not negative anywhere, so its signs say nothing, and it is read by the dense kernels only)", i);
    read_conv_keys(s, L);
    if (L.filters < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: conv filters %d", i, L.filters);
    if (L.size < 1 || L.size > CONV_MAX_SIZE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: xnor conv size %d (1..%d are served)", i, L.size, CONV_MAX_SIZE);
    if (L.stride < 1 || L.pad < 0) return fail(c, YOLO_ERR_INVALID, "layer %d: conv stride %d, padding %d", i, L.stride, L.pad);
    if (k.H + 2 * L.pad < L.size || k.W + 2 * L.pad < L.size) return fail(c, YOLO_ERR_INVALID, "layer %d: conv larger than its padded input (%d x %d with padding %d under a size %d conv)", i, k.W, k.H, L.pad, L.size);
    if (int r = side_conv_tail(k, s, L)) return r;
    conv_out(k, L);
    conv_totals(c, L, L.cin, k.H, k.W);
    return YOLO_OK;
}

static int parse_convolutional(Cursor &k, const Section &s, Layer &L)
{
    if (opt_i(s, "xnor", 0)) return parse_xnor_conv(k, s, L);
    if (opt_i(s, "groups", 1) != 1) return parse_grouped_conv(k, s, L);
    yolo_ctx *c = k.c; const int i = k.i;
    // (the variable: A/B of the dense kernels against the grouped kernel run with one group, tools/wide_conv_rate.py -- wherever that kernel serves the layer)
    if (getenv("YOLO_DENSE_AS_GROUPED") && i > 0 && opt_i(s, "size", 1) > 3 && opt_i(s, "size", 1) <= GCONV_MAX_SIZE && c->dtype != YOLO_FP8 && !c->split()) return parse_grouped_conv(k, s, L);
    L.type = L_CONV; read_conv_keys(s, L);
    if (int r = plan_activation(c, i, s, "logistic", false)) return r;
    if (L.size == 7 && L.stride == 2 && L.pad == 3 && i == 0 && k.C == 3 && k.H % 2 == 0 && k.W % 2 == 0 && c->dtype != YOLO_FP8) L.s2d7 = true;
    else if (L.size != 1 && L.size != 3) {
        // any size 1..CONV_MAX_SIZE in bf16, fp16 and fp32 (up to 25 taps: one validity bit per tap; more: row / column masks, conv_wide.hip;
        // fp32: per-tap bounds tests).  The e4m3 kernels and the pair K loop (uniform taps only) keep sizes 1 and 3
        if (c->dtype == YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: conv size %d unsupported on the device path", i, L.size);
        if (L.size < 1 || L.size > CONV_MAX_SIZE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: conv size %d (1..%d are served)", i, L.size, CONV_MAX_SIZE);
        if (c->split()) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: conv size %d is not served in the split-fp16 configuration (sizes 1 and 3, and a 7x7 / stride 2 first layer)", i, L.size);
    }
    // padding= is taken literally when pad=0, and any stride: the tiled kernels serve both; what has no output pixel is refused
    if (L.filters < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: conv filters %d", i, L.filters);
    if (L.stride < 1 || L.pad < 0) return fail(c, YOLO_ERR_INVALID, "layer %d: conv stride %d, padding %d", i, L.stride, L.pad);
    if (k.H + 2 * L.pad < L.size || k.W + 2 * L.pad < L.size) return fail(c, YOLO_ERR_INVALID, "layer %d: conv larger than its padded input (%d x %d with padding %d under a size %d conv)", i, k.W, k.H, L.pad, L.size);
    // fp8 mode: the first conv still reads the bf16 image (3 real channels padded to 8) with bf16 filters; a conv reads its
    // producer's tensor in the type that tensor is stored in (cfg key `yolo_store=bf16` on a [convolutional] section of an fp8
    // network keeps that layer's output -- and what is derived from it without arithmetic -- in bf16: mixed-precision plans)
    L.in_dt = c->dtype == YOLO_FP8 ? (i == 0 ? DT_BF16 : c->layers[i - 1].store_dt) : c->act_dt();
    L.store_dt = c->act_dt();
    const std::string st = opt_s(s, "yolo_store", "");
    if (!st.empty()) {
        if (c->dtype != YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: yolo_store is a key of fp8 networks (mixed e4m3 / bf16 plans)", i);
        if (st == "bf16") L.store_dt = DT_BF16; else if (st == "fp8") L.store_dt = DT_FP8;
        else return fail(c, YOLO_ERR_INVALID, "layer %d: yolo_store=%s (bf16 or fp8)", i, st.c_str());
    }
    L.cin = k.C; L.cin_pad = roundup(k.C, L.in_dt == DT_FP8 ? 16 : 8);
    // the conv kernel's view of a pair tensor: a layer output is interleaved per 32-channel group, 2 * roundup(C, 32) elements per
    // pixel and tap (pair K loop); the network input keeps the three blocks hi | lo | hi of its 8 padded channels (plain K loop)
    if (c->pair_of(i - 1)) L.cin_pad = i - 1 < 0 ? 3 * roundup(k.C, 8) : pair_width(k.C);
    L.pair = c->split() && opt_i(s, "yolo_pair", 1) != 0;
    L.kpad = roundup(L.size * L.size * L.cin_pad, L.in_dt == DT_FP8 ? 128 : 64); L.cout_pad = roundup(L.filters, 256);
    if (L.s2d7) { L.cin_pad = 32; L.kpad = 16 * 32; }          // 4x4 taps x (2x2 positions x 8 padded channels)
    conv_out(k, L);
    conv_totals(c, L, L.cin, k.H, k.W);
    return YOLO_OK;
}

// transposed convolution (DN/deconvolutional_layer.c, DN/parser.c:151-174), deconv.hip
static int parse_deconvolutional(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_DECONV;
    if (int r = side_conv_dtype(c, i, L)) return r;
    read_conv_keys(s, L);
    if (L.size < 1 || L.size > DECONV_MAX_SIZE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: deconv size %d (1..%d are served)", i, L.size, DECONV_MAX_SIZE);
    if (L.stride < 1 || L.stride > DECONV_MAX_STRIDE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: deconv stride %d (1..%d are served)", i, L.stride, DECONV_MAX_STRIDE);
    if (L.pad < 0 || L.pad >= L.size) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: deconv padding %d must be below its size %d", i, L.pad, L.size);
    if (L.filters < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: deconv filters %d", i, L.filters);
    const int ho = (k.H - 1) * L.stride + L.size - 2 * L.pad, wo = (k.W - 1) * L.stride + L.size - 2 * L.pad;
    if (ho < 1 || wo < 1) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: deconv output %d x %d is not positive", i, wo, ho);
    if (int r = side_conv_tail(k, s, L)) return r;
    conv_totals(c, L, L.cin, k.H, k.W);      // (over the INPUT grid: every input pixel meets every tap)
    k.H = ho; k.W = wo; k.C = L.filters;
    return YOLO_OK;
}

static int parse_connected(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    if (c->dtype == YOLO_FP8 || c->split()) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [connected] is not served in the fp8 / split-fp16 configurations", i);
    L.type = L_CONV; L.fc = true; L.fc_h = k.H; L.fc_w = k.W; L.fc_c = k.C;
    // batch_normalize=1 (DN/connected_layer.c:161: gemm, the rolling statistics, scale, bias): folded into the rows and the bias when the weights are packed, as a conv's
    L.filters = opt_i(s, "output", 1); L.size = 1; L.stride = 1; L.pad = 0; L.bn = opt_i(s, "batch_normalize", 0) != 0;
    if (L.filters < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [connected] output=%d", i, L.filters);
    if (int r = plan_activation(c, i, s, "logistic", false)) return r;
    L.in_dt = c->act_dt(); L.store_dt = c->act_dt();
    if ((long)k.H * k.W * k.C > (1L << 24)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [connected] input too large", i);
    L.cin = k.H * k.W * k.C; L.cin_pad = roundup(L.cin, 8); L.kpad = roundup(L.cin_pad, 64); L.cout_pad = roundup(L.filters, 256);
    c->conv_flops += 2.0 * L.cin * L.filters;
    c->weights_count += connected_floats(L.cin, L.filters, L.bn);
    k.H = 1; k.W = 1; k.C = L.filters;
    return YOLO_OK;
}

// [rnn] / [gru] / [lstm] (DN/parser.c:222-255): `output` units over the flattened producer, which they read as a [connected] layer does; one call
// of the library is one time step (darknet after set_batch_network(net, 1) with time_steps=1), batch index b is stream b.  Their sublayers are
// [connected] layers (file order: recur_sublayers); which launches they become: recur_geom.  fp8 / split-fp16: refused by parse_sections
static bool is_recurrent(const std::string &t) { return t == "rnn" || t == "gru" || t == "lstm" || t == "crnn"; }
static int parse_recurrent(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_RECUR; L.rkind = s.type == "rnn" ? RECUR_RNN : s.type == "gru" ? RECUR_GRU : RECUR_LSTM;
    L.filters = opt_i(s, "output", 1); L.size = 1; L.stride = 1; L.pad = 0; L.bn = opt_i(s, "batch_normalize", 0) != 0;
    if (L.filters < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [%s] output=%d", i, s.type.c_str(), L.filters);
    if (L.rkind == RECUR_RNN) {          // any activation: the kernel's epilogue applies it to each product before the sum
        const std::string name = opt_s(s, "activation", "logistic");
        L.act = act_from_name(name.c_str()); L.rshortcut = opt_i(s, "shortcut", 0) != 0;
        if (L.act < 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: activation '%s' unsupported", i, name.c_str());
    }
    if (L.rkind == RECUR_GRU) L.rtanh = opt_i(s, "tanh", 0) != 0;
    if ((long)k.H * k.W * k.C > (1L << 24)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [%s] input too large", i, s.type.c_str());
    L.fc_h = k.H; L.fc_w = k.W; L.fc_c = k.C; L.cin = k.H * k.W * k.C;
    L.in_dt = c->act_dt(); L.store_dt = c->act_dt();
    int subs[8]; const int ns = recur_sublayers(L, subs);
    for (int q = 0; q < ns; ++q) { const int inputs = subs[q] ? L.filters : L.cin; c->conv_flops += 2.0 * inputs * L.filters; c->weights_count += connected_floats(inputs, L.filters, L.bn); }
    k.H = 1; k.W = 1; k.C = L.filters;
    return YOLO_OK;
}

// locally connected (DN/local_layer.c; darknet's own yolov1.cfg): `pad` is a flag AND the im2col pad amount (:10-24, :103)
static int parse_local(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    if (c->dtype == YOLO_FP8 || c->split()) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [local] is not served in the fp8 / split-fp16 configurations", i);
    L.type = L_LOCAL; L.filters = opt_i(s, "filters", 1); L.size = opt_i(s, "size", 1); L.stride = opt_i(s, "stride", 1); L.pad = opt_i(s, "pad", 0);
    if (L.pad != 0 && L.pad != 1) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [local] pad must be 0 or 1", i);
    // pad=1 pads by ONE pixel whatever the size (DN/local_layer.c:103 im2col) while the output size assumes size / 2 (:10-24): they only agree for 3x3
    if (L.pad == 1 && L.size != 3) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [local] with pad=1 needs size=3 (darknet's own output size and im2col disagree otherwise)", i);
    if (int r = plan_activation(c, i, s, "logistic", false)) return r;
    if (k.C % 8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [local] needs a producer with a multiple of 8 channels", i);
    L.cin = k.C; L.cin_pad = k.C; L.in_dt = c->act_dt(); L.store_dt = c->act_dt();
    const int ho = ((L.pad ? k.H - 1 : k.H - L.size)) / L.stride + 1, wo = ((L.pad ? k.W - 1 : k.W - L.size)) / L.stride + 1;
    if (ho < 1 || wo < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [local] larger than its input", i);
    k.H = ho; k.W = wo; k.C = L.filters;
    c->conv_flops += 2.0 * L.size * L.size * L.cin * L.filters * (double)k.H * k.W;
    c->weights_count += (size_t)L.filters * k.H * k.W + (size_t)k.H * k.W * L.filters * L.cin * L.size * L.size;
    return YOLO_OK;
}

// [crnn] (DN/crnn_layer.c:29-130, DN/parser.c:207-220): state' = [shortcut ? state : 0] + act(conv_in(x)) + act(conv_self(state)), out = act(conv_out(state')),
// three 3x3 / stride 1 / pad 1 convs with the section's activation and batch norm.  Planned as three launches of the dense conv kernels through
// their own selection rule (run_crnn): conv_in with the old state as its epilogue's residual (shortcut=1), conv_self with conv_in's result as its
// residual, conv_out.  The residual is added behind the activation: with an activation the conv epilogue does not apply itself (logistic, the section's
// default, tanh, ...) each conv is followed by k_activate and, where it sums, an add launch
static int parse_crnn(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    const int hidden = opt_i(s, "hidden_filters", 1), output = opt_i(s, "output_filters", 1);
    if (hidden < 1 || output < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [crnn] hidden_filters=%d output_filters=%d", i, hidden, output);
    // DN/parser.c:215 hands make_crnn_layer (w, h) where it takes (h, w): the reference's own layer is only meaningful on a square map
    if (k.H != k.W) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [crnn] over a %d x %d map: the reference builds the layer with height and width exchanged, so only a square map is served", i, k.W, k.H);
    if (i == 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [crnn] as the network's first layer is not served", i);
    L.type = L_CRNN; L.filters = output; L.cin = hidden; L.size = 3; L.stride = 1; L.pad = 1; L.bn = opt_i(s, "batch_normalize", 0) != 0; L.rshortcut = opt_i(s, "shortcut", 0) != 0;
    const std::string name = opt_s(s, "activation", "logistic");
    L.act = act_from_name(name.c_str());
    if (L.act < 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: activation '%s' unsupported", i, name.c_str());
    L.in_dt = c->act_dt(); L.store_dt = c->act_dt();
    const int cins[3] = {k.C, hidden, hidden}, couts[3] = {hidden, hidden, output};
    L.sub.assign(3, Layer());
    for (int q = 0; q < 3; ++q) {
        Layer &S = L.sub[q];
        S.type = L_CONV; S.filters = couts[q]; S.size = 3; S.stride = 1; S.pad = 1; S.bn = L.bn; S.act = L.act; S.in_dt = S.store_dt = c->act_dt();
        S.cin = cins[q]; S.cin_pad = roundup(S.cin, 8); S.kpad = roundup(9 * S.cin_pad, 64); S.cout_pad = roundup(S.filters, 256);
        S.H = k.H; S.W = k.W; S.C = S.filters;
        conv_totals(c, S, S.cin, k.H, k.W);
    }
    k.C = output;
    return YOLO_OK;
}

// [dropout] (DN/dropout_layer.c:38-40) and [cost] (DN/cost_layer.c: forward returns without a truth): the identity at inference
static int parse_identity(Cursor &, const Section &s, Layer &L) { L.type = L_ROUTE; L.cost = s.type == "cost"; return YOLO_OK; }

static int parse_detection(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_DETECT; L.classes = opt_i(s, "classes", 1); L.na = opt_i(s, "num", 1); L.side = opt_i(s, "side", 7); L.sqr = opt_i(s, "sqrt", 0);
    if (opt_i(s, "coords", 4) != 4 || opt_i(s, "softmax", 0)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [detection] with coords != 4 or softmax", i);
    if (int r = side_conv_before_head(c, i, "detection", "[detection] must follow a [connected] layer", "[detection] must follow a [connected] layer")) return r;
    if (i == 0 || !c->layers[i - 1].fc) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [detection] must follow a [connected] layer", i);
    if (k.C != L.side * L.side * (L.classes + L.na * 5)) return fail(c, YOLO_ERR_INVALID, "layer %d: [detection] expects %d inputs, got %d", i, L.side * L.side * (L.classes + L.na * 5), k.C);
    if (c->attrs && c->attrs != 5 + L.classes) return fail(c, YOLO_ERR_UNSUPPORTED, "heads with different class counts");
    c->attrs = 5 + L.classes; L.row_off = c->rows; c->rows += L.side * L.side * L.na;
    if (c->layers[i - 1].post_act != ACT_LINEAR) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: the layer in front of a [detection] head needs a linear, leaky, relu or relie activation", i - 1);
    c->layers[i - 1].head = true;
    k.H = L.side; k.W = L.side;
    return YOLO_OK;
}

static int parse_shortcut(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_SHORTCUT; int f = opt_i(s, "from", -1); f = f < 0 ? i + f : f;
    if (f < 0 || f >= i) return fail(c, YOLO_ERR_INVALID, "layer %d: bad shortcut from", i);
    L.in = {i - 1, f};
    if (int r = plan_activation(c, i, s, "linear", true)) return r;
    // the general form (DN/blas.c:68-92 shortcut_cpu): a `from` tensor of another channel count or size, or an activation.  (w1, h1,
    // c1) = the `from` tensor, (w2, h2, c2) = this layer's input and output; the reference asserts what is checked here
    int h1, w1, c1; k.dims(f, h1, w1, c1);
    L.general = h1 != k.H || w1 != k.W || c1 != k.C || L.act != ACT_LINEAR;
    if (!shortcut_geom(w1, h1, c1, k.W, k.H, k.C).ok)
        return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: shortcut of a %d x %d tensor (layer %d) into a %d x %d one: darknet requires w1 / w2 == h1 / h2 and w2 / w1 == h2 / h1", i, w1, h1, f, k.W, k.H);
    if (L.general && c->dtype == YOLO_FP8)
        return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: a [shortcut] with an activation or a `from` tensor of another shape is not served in the fp8 configuration", i);
    return YOLO_OK;
}

static int parse_route(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_ROUTE; L.in.clear();
    std::vector<float> ls = opt_list(s, "layers");
    if (ls.empty()) return fail(c, YOLO_ERR_INVALID, "layer %d: route without layers", i);
    k.C = 0;
    for (float v : ls) {
        int l = (int)v; l = l < 0 ? i + l : l;
        if (l < 0 || l >= i) return fail(c, YOLO_ERR_INVALID, "layer %d: bad route index", i);
        L.in.push_back(l);
        int h2, w2, c2; k.dims(l, h2, w2, c2);
        if (L.in.size() == 1) { k.H = h2; k.W = w2; } else if (h2 != k.H || w2 != k.W) return fail(c, YOLO_ERR_INVALID, "layer %d: route spatial mismatch", i);
        k.C += c2;
    }
    return YOLO_OK;
}

// TF semantics: the 2x bilinear closed form only.  darknet semantics (DN/upsample_layer.c): nearest, any stride 1..8; a stride
// below 1 is darknet's reverse mode, which is not served.  scale= (out = scale * in) in both
static int parse_upsample(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_UPSAMPLE; L.pstride = opt_i(s, "stride", 2); L.up_scale = (float)atof(opt_s(s, "scale", "1").c_str());
    if (c->semantics == YOLO_SEM_DARKNET ? (L.pstride < 1 || L.pstride > 8) : L.pstride != 2) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: upsample stride %d", i, L.pstride);
    if ((L.pstride != 2 || L.up_scale != 1.f) && (c->dtype == YOLO_FP8 || c->split()))
        return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [upsample] with a stride other than 2 or a scale is not served in the fp8 / split-fp16 configurations", i);
    k.H *= L.pstride; k.W *= L.pstride;
    return YOLO_OK;
}

// [logistic] / [activation] (DN/logistic_layer.c, DN/activation_layer.c): activate_array over a copy of the input -- here k_activate over the producer's tensor
static int parse_activate(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    if (c->dtype == YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [%s] is not served in the fp8 configuration", i, s.type.c_str());
    L.type = L_ACTIVATE;
    if (s.type == "logistic") L.act = ACT_LOGISTIC;
    else if (int r = plan_activation(c, i, s, "linear", true)) return r;
    return YOLO_OK;
}

static int parse_l2norm(Cursor &k, const Section &, Layer &L)
{
    if (k.c->dtype == YOLO_FP8 || k.c->split()) return fail(k.c, YOLO_ERR_UNSUPPORTED, "layer %d: [l2norm] is not served in the fp8 / split-fp16 configurations", k.i);
    L.type = L_L2NORM;
    return YOLO_OK;
}

// [normalization] / [lrn] (DN/parser.c:511-519, DN/normalization_layer.c): local response normalisation over the channels, shape in = shape out, stored in its
// input's type.  The reference's initial loop reads the channels 0 .. size / 2 - 1 whatever C is: size / 2 > C reads past the image there and is refused here
static int parse_normalization(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i; const char *name = s.type.c_str();
    if (c->dtype == YOLO_FP8 || c->split()) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [%s] is not served in the fp8 / split-fp16 configurations", i, name);
    L.type = L_LRN; L.size = opt_i(s, "size", 5);
    L.lrn_alpha = (float)atof(opt_s(s, "alpha", ".0001").c_str()); L.lrn_beta = (float)atof(opt_s(s, "beta", ".75").c_str()); L.lrn_kappa = (float)atof(opt_s(s, "kappa", "1").c_str());
    if (L.size < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [%s] size=%d", i, name, L.size);
    if (L.size > LRN_MAX_SIZE) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [%s] size=%d (1..%d are served)", i, name, L.size, LRN_MAX_SIZE);
    if (L.size / 2 > k.C) return fail(c, YOLO_ERR_INVALID, "layer %d: [%s] size=%d over %d channels: size / 2 must not exceed the channel count (the reference reads past the image)", i, name, L.size, k.C);
    return YOLO_OK;
}

// [crop] at inference (DN/parser.c:429-451, DN/crop_layer.c:67-102 with net.train == 0): the centred crop_height x crop_width window, times 2 minus 1 unless
// noadjust=1.  flip / angle / saturation / exposure / shift act while training only: read by nobody.  It may be layer 0 (darknet's own classifier cfgs): the
// conv behind it then reads a 3-channel layer tensor through the tiled kernel -- the fused stems ask for a conv at layer 0
static int parse_crop(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    if (c->dtype == YOLO_FP8 || c->split()) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [crop] is not served in the fp8 / split-fp16 configurations", i);
    const int ch = opt_i(s, "crop_height", 1), cw = opt_i(s, "crop_width", 1);
    L.type = L_CROP; L.crop_adjust = opt_i(s, "noadjust", 0) == 0;
    if (ch < 1 || cw < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [crop] crop_height=%d crop_width=%d", i, ch, cw);
    if (ch > k.H || cw > k.W) return fail(c, YOLO_ERR_INVALID, "layer %d: [crop] to %d x %d is larger than its %d x %d input (the reference reads out of bounds)", i, cw, ch, k.W, k.H);
    k.H = ch; k.W = cw;
    return YOLO_OK;
}

static int parse_maxpool(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_MAXPOOL; L.pstride = opt_i(s, "stride", 1); L.psize = opt_i(s, "size", L.pstride);
    L.ppad = opt_i(s, "padding", (L.psize - 1) / 2);
    if (L.pstride < 1 || L.psize < 1 || L.ppad < 0) return fail(c, YOLO_ERR_INVALID, "layer %d: [maxpool] size %d, stride %d, padding %d", i, L.psize, L.pstride, L.ppad);
    k.H = (k.H + 2 * L.ppad) / L.pstride; k.W = (k.W + 2 * L.ppad) / L.pstride;
    if (k.H < 1 || k.W < 1) return fail(c, YOLO_ERR_INVALID, "layer %d: [maxpool] with stride %d leaves no output pixel", i, L.pstride);
    return YOLO_OK;
}

static int parse_reorg(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = L_REORG; L.pstride = opt_i(s, "stride", 1);
    if (L.pstride < 1 || k.H % L.pstride || k.W % L.pstride) return fail(c, YOLO_ERR_INVALID, "layer %d: reorg stride", i);
    // darknet's reorg_cpu takes channel indices modulo c / stride^2 (DN/blas.c:9-30): with fewer channels than stride^2 it divides by zero
    if (c->semantics == YOLO_SEM_DARKNET && k.C < L.pstride * L.pstride) return fail(c, YOLO_ERR_INVALID, "layer %d: [reorg] with stride %d needs at least %d channels in darknet semantics (its producer has %d)", i, L.pstride, L.pstride * L.pstride, k.C);
    k.H /= L.pstride; k.W /= L.pstride; k.C *= L.pstride * L.pstride;
    return YOLO_OK;
}

// [yolo] / [region]: the anchors (masked for [yolo]), the rows the head adds, `head` on the conv in front of it
static int parse_head(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    L.type = s.type == "yolo" ? L_YOLO : L_REGION;
    L.classes = opt_i(s, "classes", 20);
    std::vector<float> an = opt_list(s, "anchors"), mask = opt_list(s, "mask");
    int total = opt_i(s, "num", 1);
    if ((int)an.size() < 2 * total) return fail(c, YOLO_ERR_INVALID, "layer %d: anchors/num mismatch", i);
    if (L.type == L_YOLO && !mask.empty()) { for (float m : mask) { int a = (int)m; if (a < 0 || a >= total) return fail(c, YOLO_ERR_INVALID, "layer %d: mask", i); L.anchors.push_back(an[2 * a]); L.anchors.push_back(an[2 * a + 1]); } }
    else L.anchors.assign(an.begin(), an.begin() + 2 * total);
    L.na = (int)L.anchors.size() / 2;
    if (L.na > 16) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: more than 16 anchors", i);
    if (int r = side_conv_before_head(c, i, s.type.c_str(), "the head's objectness plane and lean decode belong to the dense kernels; put a dense 1x1 conv in between",
                                      "the head's fp32 store, objectness plane and lean decode belong to the dense kernels; put a dense 1x1 conv in between")) return r;
    if (i == 0 || c->layers[i - 1].type != L_CONV) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: head must follow a conv", i);
    if (k.C != L.na * (5 + L.classes)) return fail(c, YOLO_ERR_INVALID, "layer %d: head expects %d channels, conv gives %d", i, L.na * (5 + L.classes), k.C);
    if (c->attrs && c->attrs != 5 + L.classes) return fail(c, YOLO_ERR_UNSUPPORTED, "heads with different class counts");
    if (L.type == L_REGION && s.kv.count("tree")) {
        // [region] with a softmax tree (YOLO9000, DN/region_layer.c:171-181): the tree takes precedence over softmax=1
        if (opt_i(s, "background", 0)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [region] tree= with background=1 is not served", i);
        if (opt_i(s, "coords", 4) != 4) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [region] tree= with coords != 4 is not served", i);
        if (s.kv.count("map")) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [region] tree= with map= in the cfg is not served (pass the map to yolo_darknet_boxes_map)", i);
        if (c->rows) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: a [region] head with a tree must be the network's only head", i);
        if (int r = plan_tree(c, i, "region", opt_s(s, "tree", ""), L.classes, "classes")) return r;
        c->tree_head = i;
    } else if (c->tree_head >= 0) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: a [region] head with a tree must be the network's only head", i);
    c->attrs = 5 + L.classes; L.row_off = c->rows; c->rows += k.H * k.W * L.na;
    if (c->layers[i - 1].post_act != ACT_LINEAR) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: the conv in front of a [yolo] / [region] head needs a linear, leaky, relu or relie activation", i - 1);
    c->layers[i - 1].head = true;
    return YOLO_OK;
}

// always global (DN/avgpool_layer.c:40-55): H x W x C -> 1 x 1 x C, stored in the form of its input
static int parse_avgpool(Cursor &k, const Section &, Layer &L)
{
    if (k.c->dtype == YOLO_FP8) return fail(k.c, YOLO_ERR_UNSUPPORTED, "layer %d: [avgpool] is not served in the fp8 configuration", k.i);
    L.type = L_AVGPOOL; k.H = 1; k.W = 1;
    return YOLO_OK;
}

// DN/parser.c:268-280: groups, temperature; per image and group e = exp(x / temp - max / temp), p = e / sum (DN/blas.c:305-321)
static int parse_softmax(Cursor &k, const Section &s, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    if (c->dtype == YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [softmax] is not served in the fp8 configuration", i);
    if (opt_i(s, "spatial", 0)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [softmax] with spatial=1 is not served", i);
    L.type = L_SOFTMAX; L.groups = opt_i(s, "groups", 1); L.temperature = L.cfg_temperature = (float)atof(opt_s(s, "temperature", "1").c_str());          // (cfg_temperature: what yolo_reset_temperature hands back)
    if (k.H != 1 || k.W != 1) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [softmax] over a %d x %d map (it must follow an [avgpool] or a [connected] layer)", i, k.H, k.W);
    if (!(L.temperature > 0.f)) return fail(c, YOLO_ERR_INVALID, "layer %d: [softmax] temperature must be > 0", i);
    if (s.kv.count("tree")) {
        // hierarchical softmax (DN/softmax_layer.c:41-48): one softmax per group of the tree, whatever `groups` says
        if (int r = plan_tree(c, i, "softmax", opt_s(s, "tree", ""), k.C, "inputs")) return r;
        L.groups = 1;
    } else {
        if (L.groups < 1 || k.C % L.groups) return fail(c, YOLO_ERR_INVALID, "layer %d: [softmax] groups=%d does not divide its %d inputs", i, L.groups, k.C);
        if (k.C / L.groups > CLS_SOFTMAX_MAX) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [softmax] group of %d logits (at most %d)", i, k.C / L.groups, CLS_SOFTMAX_MAX);
    }
    // the logits are never rounded to 16 bits: the conv that reaches this layer directly, or through one [avgpool], writes fp32
    int p = i - 1;
    if (p >= 0 && c->layers[p].type == L_AVGPOOL) p = c->layers[p].in[0];
    if (p >= 0 && (c->layers[p].type == L_CONV || (is_side_conv(c->layers[p]) && c->layers[p].type != L_DECONV) || c->layers[p].type == L_RECUR)) c->layers[p].head = true;      // (not L_DECONV)
    return YOLO_OK;
}

static const struct { const char *name; int (*parse)(Cursor &, const Section &, Layer &); } section_table[] = {
    {"convolutional", parse_convolutional}, {"connected", parse_connected}, {"local", parse_local}, {"dropout", parse_identity}, {"detection", parse_detection},
    {"shortcut", parse_shortcut}, {"route", parse_route}, {"upsample", parse_upsample}, {"deconvolutional", parse_deconvolutional},
    {"logistic", parse_activate}, {"activation", parse_activate}, {"l2norm", parse_l2norm}, {"maxpool", parse_maxpool}, {"reorg", parse_reorg},
    {"yolo", parse_head}, {"region", parse_head}, {"avgpool", parse_avgpool}, {"softmax", parse_softmax}, {"cost", parse_identity},
    {"rnn", parse_recurrent}, {"gru", parse_recurrent}, {"lstm", parse_recurrent}, {"crnn", parse_crnn},
    {"normalization", parse_normalization}, {"lrn", parse_normalization}, {"crop", parse_crop},
};

// After each section: a layer that moves data keeps the type and the pair form of what it moves, and its operands must agree.
// Reads store_dt / pair of the layers in L.in, L.general; writes L.store_dt, L.pair
static int inherit_form(const Cursor &k, Layer &L)
{
    yolo_ctx *c = k.c; const int i = k.i;
    if (computes(L) || L.type == L_LOCAL) return YOLO_OK;
    int dt = -1;
    for (int j : L.in) { const int dj = j < 0 ? c->act_dt() : c->layers[j].store_dt; if (dt >= 0 && dj != dt && (L.type == L_ROUTE || L.type == L_SHORTCUT)) return fail(c, YOLO_ERR_INVALID, "layer %d: operands stored in different types (yolo_store): a %s needs one type", i, L.type == L_ROUTE ? "route" : "shortcut"); if (dt < 0) dt = dj; }
    L.store_dt = dt >= 0 ? dt : c->act_dt();
    if (c->split() && !L.in.empty() && !is_head_layer(L)) {
        L.pair = c->pair_of(L.in[0]);
        for (int j : L.in) if (c->pair_of(j) != L.pair) return fail(c, YOLO_ERR_INVALID, "layer %d: operands stored in different forms (yolo_pair): a %s needs pairs or plain fp16 throughout", i, L.type == L_ROUTE ? "route" : L.type == L_SHORTCUT ? "shortcut" : "layer");
        // pairs are interleaved per 32-channel group: the general shortcut's channel boundary (minc) must fall between groups
        // ... and a [reorg] scrambles channels across them: whole groups in, whole groups out (via_f32)
        if (L.type == L_REORG && L.pair) { int h1, w1, c1; k.dims(L.in[0], h1, w1, c1); if (c1 % 32 || L.C % 32) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: a [reorg] of split-fp16 pairs needs a channel count that is a multiple of 32 (%d)", i, c1); }
        if (L.type == L_SHORTCUT && L.general && L.pair) { int h1, w1, c1; k.dims(L.in[1], h1, w1, c1); if (L.C % 32 || c1 % 32) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: a [shortcut] with an activation or a `from` tensor of another shape, on split-fp16 pairs, needs channel counts that are multiples of 32 (%d and %d)", i, L.C, c1); }
    }
    return YOLO_OK;
}

// [net] keys of the input, the layer array, the pair form of the image; then every section through section_table and inherit_form.
// Writes in_h / in_w / in_c / in_pair, the totals, and per layer everything the parsers and inherit_form write plus in[] and H / W / C
static int parse_sections(yolo_ctx *c, const std::vector<Section> &secs)
{
    const Section &net = secs[0];
    c->in_h = opt_i(net, "height", 0); c->in_w = opt_i(net, "width", 0); c->in_c = opt_i(net, "channels", 3);
    // [net] yolo_input=vector with inputs=N (char-rnn: DN/parser.c:656 net->inputs where the cfg names no image size): the input is one row of N values per stream.
    // Without the key a cfg without a size stays refused, as before
    const std::string in_kind = opt_s(net, "yolo_input", "");
    if (!in_kind.empty() && in_kind != "vector" && in_kind != "planes") return fail(c, YOLO_ERR_INVALID, "cfg: yolo_input=%s (the values are `vector` and `planes`)", in_kind.c_str());
    c->vec_n = 0;
    if (in_kind == "vector") {
        const int N = opt_i(net, "inputs", 0);
        if (c->in_h > 0 || c->in_w > 0) return fail(c, YOLO_ERR_INVALID, "cfg: yolo_input=vector together with height=%d / width=%d: a vector network has no image size (inputs= alone gives its length)", c->in_h, c->in_w);
        if (N <= 0 || N > (1 << 24)) return fail(c, YOLO_ERR_INVALID, "cfg: yolo_input=vector needs inputs= of 1..%d (got %d)", 1 << 24, N);
        if (!opt_s(net, "yolo_output", "").empty()) return fail(c, YOLO_ERR_UNSUPPORTED, "cfg: yolo_input=vector together with yolo_output=map is not served");
        c->vec_n = N; c->in_h = 1; c->in_w = 1; c->in_c = N;
    } else if (in_kind == "planes") {
        // [net] yolo_input=planes with height, width and channels=N: an image network of N planes (grey, RGB-D, multispectral, darknet's go board).  With
        // channels=3 the plan is the plan of the cfg without the key; any other count is staged as roundup(N, 8) channels per pixel and read by layer 0 as
        // any inner layer reads a tensor of N channels
        if (c->in_h <= 0 || c->in_w <= 0) {
            if (net.kv.count("inputs")) return fail(c, YOLO_ERR_INVALID, "cfg: yolo_input=planes with inputs=%d and no image size: it needs positive height= and width= (got height=%d width=%d)", opt_i(net, "inputs", 0), c->in_h, c->in_w);
            return fail(c, YOLO_ERR_INVALID, "cfg: yolo_input=planes needs positive height= and width= (got height=%d width=%d)", c->in_h, c->in_w);
        }
        if (c->in_c < 1 || c->in_c > PLANES_MAX) return fail(c, YOLO_ERR_INVALID, "cfg: yolo_input=planes needs channels= of 1..%d (got channels=%d)", PLANES_MAX, c->in_c);
        if (c->in_c != 3 && (c->dtype == YOLO_FP8 || c->split()))
            return fail(c, YOLO_ERR_UNSUPPORTED, "cfg: yolo_input=planes with channels=%d is not served in the %s configuration (bf16, fp16 and fp32 are)", c->in_c, c->split() ? "split-fp16" : "fp8");
    } else if (c->in_h <= 0 || c->in_w <= 0 || c->in_c != 3)
        return fail(c, YOLO_ERR_UNSUPPORTED, "cfg: need an input of positive height and width with 3 channels (got %dx%dx%d); a vector-input network ([net] inputs=N, no image size) is declared with [net] yolo_input=vector, an image network of another channel count with [net] yolo_input=planes", c->in_w, c->in_h, c->in_c);
    const int NL = (int)secs.size() - 1;
    // a recurrent layer is served in the bf16, fp16 and fp32 configurations: refused here, by its own name, ahead of whatever else of such a network the
    // configuration refuses.  ([net] time_steps is read and ignored: one call is one step)
    for (int i = 0; i < NL && (c->dtype == YOLO_FP8 || c->split()); ++i)
        if (is_recurrent(secs[i + 1].type)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [%s] is not served in the %s configuration", i, secs[i + 1].type.c_str(), c->split() ? "split-fp16" : "fp8");
    if (c->vec_n && (c->dtype == YOLO_FP8 || c->split()))
        return fail(c, YOLO_ERR_UNSUPPORTED, "cfg: a vector-input network (yolo_input=vector) is not served in the %s configuration (bf16, fp16 and fp32 are)", c->split() ? "split-fp16" : "fp8");
    // ... and serves the sections that read a row of values; the others are refused here, by name
    static const char *const vector_sections[] = {"connected", "rnn", "gru", "lstm", "dropout", "activation", "softmax", "cost"};
    for (int i = 0; i < NL && c->vec_n; ++i)
        if (std::none_of(std::begin(vector_sections), std::end(vector_sections), [&](const char *t) { return secs[i + 1].type == t; }))
            return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [%s] needs an image-shaped input: a vector-input network (yolo_input=vector) serves [connected], [rnn], [gru], [lstm], [dropout], [activation], [softmax] and [cost]", i, secs[i + 1].type.c_str());
    c->layers.resize(NL);
    c->rows = 0; c->attrs = 0; c->conv_flops = 0; c->weights_count = 0;
    // split-fp16 networks: per-tensor storage form (mixed plans): pairs unless a [convolutional] section says yolo_pair=0
    // ([net] yolo_pair_input for the image); layers that move data inherit, both operands of a shortcut / all inputs of a route must agree
    c->in_pair = c->split() && opt_i(net, "yolo_pair_input", 1) != 0;
    // (a 7x7 / stride 2 first conv reads the 2x2 space-to-depth of the image, which is kept as plain fp16: such a network's input is never pairs)
    if (c->in_pair && NL >= 1 && secs[1].type == "convolutional" && opt_i(secs[1], "size", 1) == 7 && opt_i(secs[1], "stride", 1) == 2) c->in_pair = false;
    Cursor k{c, 0, c->in_h, c->in_w, c->in_c};
    for (k.i = 0; k.i < NL; ++k.i) {
        const Section &s = secs[k.i + 1]; Layer &L = c->layers[k.i];
        L.in = {k.i - 1};
        if (!c->split() && (s.kv.count("yolo_pair") || net.kv.count("yolo_pair_input"))) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: yolo_pair is a key of split-fp16 networks (YOLO_FP16X2)", k.i);
        const auto *e = std::find_if(std::begin(section_table), std::end(section_table), [&](const auto &t) { return s.type == t.name; });
        if (e == std::end(section_table)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: section [%s] is outside the inference hot path", k.i, s.type.c_str());
        if (int r = e->parse(k, s, L)) return r;
        L.H = k.H; L.W = k.W; L.C = k.C;
        if (int r = inherit_form(k, L)) return r;
    }
    return YOLO_OK;
}

// ---- after the sections, in this order (each reads what the ones above it wrote) ----------------------------------------------
// heads are fp32.  Reads head; writes pair
static void heads_to_fp32(yolo_ctx *c) { for (Layer &L : c->layers) if (L.head) L.pair = false; }

// classifier tail: an [avgpool] of an fp32 logit map stays fp32 and is pooled inside the [softmax] launch behind it; a [softmax] reads fp32.
// Reads head (of the producer), tree, C; writes pair, store_dt, pool_fused
static int classifier_tail(yolo_ctx *c)
{
    const int NL = (int)c->layers.size();
    for (int i = 0; i < NL; ++i) {
        Layer &L = c->layers[i];
        const int j = L.in.empty() ? -1 : L.in[0];
        if (L.type == L_AVGPOOL && (c->dtype == YOLO_FP32 || (j >= 0 && c->layers[j].head))) {
            L.pair = false; L.store_dt = DT_F32;
            L.pool_fused = i + 1 < NL && c->layers[i + 1].type == L_SOFTMAX && c->layers[i + 1].tree < 0 && L.C <= CLS_SOFTMAX_MAX && !getenv("YOLO_NO_POOL_FUSE");
        }
        if (L.type == L_SOFTMAX) {
            L.pair = false; L.store_dt = DT_F32;
            if (!(c->dtype == YOLO_FP32 || (j >= 0 && (c->layers[j].head || (c->layers[j].type == L_AVGPOOL && c->layers[j].store_dt == DT_F32)))))
                return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [softmax] must follow a [convolutional] / [connected] layer, directly or through one [avgpool] (fp32 logits)", i);
        }
    }
    return YOLO_OK;
}

// the kind of network: a detector (rows > 0), else a map where [net] yolo_output=map declares one (the image-shaped tensor of the last layer
// that is not [cost]), else a classifier (that layer is a [softmax]).  Reads rows, cost, type; writes map_layer / cls_layer, head and pair along the map chain
static int network_kind(yolo_ctx *c, const Section &net)
{
    const std::string out_kind = opt_s(net, "yolo_output", "");
    if (!out_kind.empty() && out_kind != "map") return fail(c, YOLO_ERR_INVALID, "cfg: yolo_output=%s (the one value is `map`)", out_kind.c_str());
    if (!out_kind.empty() && c->rows) return fail(c, YOLO_ERR_INVALID, "cfg: yolo_output=map on a network with a [yolo] / [region] / [detection] head");
    if (c->rows) return YOLO_OK;
    int o = (int)c->layers.size() - 1;
    while (o >= 0 && c->layers[o].cost) --o;
    if (out_kind.empty()) {
        if (c->vec_n && (o < 0 || c->layers[o].type != L_SOFTMAX)) return fail(c, YOLO_ERR_INVALID, "cfg: the output layer of a vector-input network (its last layer that is not [cost]) must be a [softmax]");
        if (o < 0 || c->layers[o].type != L_SOFTMAX) return fail(c, YOLO_ERR_INVALID, "cfg has no [yolo] / [region] / [detection] head");
        c->cls_layer = o;
        return YOLO_OK;
    }
    if (o < 0 || c->layers[o].type == L_SOFTMAX) return fail(c, YOLO_ERR_INVALID, "cfg: yolo_output=map on a network whose output layer is a [softmax] (a classifier)");
    c->map_layer = o;
    // the map is never rounded to 16 bits: the computing layer that reaches it directly or through [logistic] / [activation] layers writes
    // fp32, and so do those (the `head` flag, as for logits)
    int p = o;
    while (p >= 0 && c->layers[p].type == L_ACTIVATE) { c->layers[p].head = true; c->layers[p].pair = false; p = c->layers[p].in[0]; }
    if (p >= 0 && computes(c->layers[p])) { c->layers[p].head = true; c->layers[p].pair = false; }
    else for (int q = o; q >= 0 && q != p; q = c->layers[q].in[0]) c->layers[q].head = false;      // (nothing computes in front of them: they keep their producer's type)
    return YOLO_OK;
}

// [net] normalisation keys and the row limit.  Reads rows; writes in_mul, in_add
static int input_norm_and_row_limit(yolo_ctx *c, const Section &net)
{
    c->in_mul = (float)atof(opt_s(net, "yolo_input_mul", "1").c_str()); c->in_add = (float)atof(opt_s(net, "yolo_input_add", "0").c_str());
    if (c->rows > 32768) return fail(c, YOLO_ERR_UNSUPPORTED, "more than 32768 candidates per image");
    return YOLO_OK;
}

// how many layers read each layer's tensor (a [shortcut] reads two, a [route] all it names)
static std::vector<int> count_uses(const yolo_ctx *c)
{
    std::vector<int> uses(c->layers.size(), 0);
    for (const Layer &L : c->layers) for (int j : L.in) if (j >= 0) uses[j]++;
    return uses;
}

// `shortcut` after a conv is folded into that conv's epilogue (V3/yolo_v3.py:54-60); the general form (k_shortcut) is never folded.
// Reads general, post_act, head, store_dt, pair, uses; writes residual_from on the conv, noop on the [shortcut]
static int fold_shortcuts(yolo_ctx *c, const std::vector<int> &uses)
{
    if (c->keep_layers) return YOLO_OK;
    for (int i = 0; i < (int)c->layers.size(); ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_SHORTCUT || L.general) continue;
        Layer &P = c->layers[i - 1];
        if (P.type == L_CONV && P.post_act == ACT_LINEAR && uses[i - 1] == 1 && !P.head && L.in[1] != i - 1 && (L.in[1] < 0 || c->layers[L.in[1]].store_dt == P.store_dt)) {
            if (c->pair_of(L.in[1]) != P.pair) return fail(c, YOLO_ERR_INVALID, "layer %d: the conv in front of this shortcut and its other operand are stored in different forms (yolo_pair)", i);
            P.residual_from = L.in[1]; L.noop = true;
        }
    }
    return YOLO_OK;
}

// ---- marking passes: each writes kernel / fused / launcher / tail_layer / fused_into of the layers it marks, nothing else ------------------
// One name per phrase the passes repeat.  A predicate stands only where the text it replaced was exactly its body; where the passes differ
// in what they ask (the stems ask no !fc, the pair stem asks no operand type, ...) they still differ.
static inline bool is16(int dt) { return dt == DT_BF16 || dt == DT_F16; }
// a layer with a post-activation runs its own plain launch, then k_activate: it is no member of a fused launch, neither end of a 1x1 tail,
// and keeps the tiled kernel.  Every marking pass asks this of each layer it marks
static inline bool plain(const Layer &X) { return X.post_act == ACT_LINEAR; }
static inline bool plain_conv(const Layer &X) { return X.type == L_CONV && plain(X) && !X.head; }      // a dense conv ([connected] included) that is plain and no head
static inline bool plain_conv_no_fc(const Layer &X) { return plain_conv(X) && !X.fc; }                  // ... and no [connected] layer
static inline bool conv_is(const Layer &X, int size, int stride, int pad) { return X.size == size && X.stride == stride && X.pad == pad; }
static inline bool hosts_shortcut(const Layer &X) { return X.residual_from >= -1; }                     // a [shortcut] was folded into it (-1: of the image)
static inline bool plain16(const Layer &X) { return is16(X.in_dt) && X.store_dt == X.in_dt && !X.pair; }      // stored in its 16-bit operand type, not pairs
static inline bool like16(const Layer &X, const Layer &A) { return X.in_dt == A.in_dt && X.store_dt == A.in_dt && !X.pair; }      // reads and stores A's operand type, not pairs
// the context may hold 16-bit tensors at all: a 16-bit network, an e4m3 one with bf16 islands (yolo_store=bf16), a split-fp16 one with plain
// fp16 islands (yolo_pair=0) -- what counts is the type of the tensors a kernel touches, not the context's
static inline bool ctx16(const yolo_ctx *c) { return c->half_like() || c->dtype == YOLO_FP8 || c->split(); }

// fused residual block (conv_block.hip): a 1x1 conv 128 -> 64 read only by the 3x3 conv 64 -> 128 that follows, whose folded shortcut
// source is the 1x1's own input, on a grid that is (nearly) whole 13 x 13 blocks: darknet-53's 104 x 104 stage at 416 x 416.
// Reads residual_from (fold_shortcuts)
static void mark_resblocks(yolo_ctx *c, const std::vector<int> &uses)
{
    const int NL = (int)c->layers.size();
    if (!(ctx16(c) && !c->keep_layers && !getenv("YOLO_NO_RESBLOCK"))) return;
    for (int i = 1; i + 1 < NL; ++i) {
        Layer &A = c->layers[i], &B = c->layers[i + 1];
        if (plain_conv_no_fc(A) && plain_conv_no_fc(B) && uses[i] == 1 && B.in[0] == i && A.in[0] >= 0 &&
            conv_is(A, 1, 1, 0) && A.cin == 128 && A.filters == 64 && B.cin == 64 && B.filters == 128 && !hosts_shortcut(A) &&
            conv_is(B, 3, 1, 1) && B.residual_from == A.in[0] &&
            ((long)((B.H + 12) / 13) * ((B.W + 12) / 13) * 169 * 100 <= (long)B.H * B.W * 115) && plain16(A) && like16(B, A) &&
            c->layers[A.in[0]].store_dt == A.in_dt && !c->pair_of(A.in[0])) { A.fused = B.fused = F_RESBLOCK; A.launcher = B.launcher = i + 1; }
    }
}

// fused stem (conv_stem.hip): conv0 (3x3/s1, 3 -> 32) read only by conv1 (3x3/s2, 32 -> 64), 16-bit, nothing asking for layer 0's tensor;
// optionally the 1x1 conv 64 -> 32 behind them.  (The stem and halo kernels address their input with 32-bit buffer offsets: the
// whole-batch window must stay under 2 GiB.)  Layer 0 reads the staged image, which is kept in its operand type
static void mark_stem(yolo_ctx *c, const std::vector<int> &uses)
{
    const int NL = (int)c->layers.size();
    if (!(ctx16(c) && !c->keep_layers && NL >= 2 && (double)c->max_batch * c->in_h * c->in_w * 8 * 2 < 2147483648.0)) return;
    const Layer &A = c->layers[0], &B = c->layers[1];
    if (!(plain_conv(A) && plain_conv(B) && uses[0] == 1 && B.in[0] == 0 && conv_is(A, 3, 1, 1) && A.cin == 3 &&
          A.filters == 32 && conv_is(B, 3, 2, 1) && B.filters == 64 && !hosts_shortcut(B) && plain16(A) && like16(B, A) && !c->in_pair)) return;
    for (int m = 0; m < 2; ++m) { c->layers[m].fused = F_STEM; c->layers[m].launcher = 1; }
    if (NL < 3) return;
    const Layer &T = c->layers[2];
    if (plain_conv_no_fc(T) && T.in[0] == 1 && conv_is(T, 1, 1, 0) && T.filters == 32 && !hosts_shortcut(T) && like16(T, A)) { c->layers[2].fused = F_STEM; c->layers[2].launcher = 1; }
}

// split-fp16: conv0 + conv1 on pairs in one launch (conv_stem_pair.hip) -- both tensors pairs, the image in its three blocks
static void mark_pair_stem(yolo_ctx *c, const std::vector<int> &uses)
{
    if (!(c->split() && !c->keep_layers && c->layers.size() >= 2 && c->in_pair && !getenv("YOLO_NO_PAIR_STEM"))) return;
    const Layer &A = c->layers[0], &B = c->layers[1];
    if (plain_conv(A) && plain_conv(B) && uses[0] == 1 && B.in[0] == 0 && conv_is(A, 3, 1, 1) && A.cin == 3 && A.bn == B.bn &&
        (A.filters == 32) && conv_is(B, 3, 2, 1) && B.filters == 64 && !hosts_shortcut(A) && !hosts_shortcut(B) &&
        A.pair && B.pair && c->in_h % 2 == 0 && c->in_w % 2 == 0 && A.kpad >= 216 && B.kpad == 576)
        for (int m = 0; m < 2; ++m) { c->layers[m].fused = F_PSTEM; c->layers[m].launcher = 1; }
}

// a conv's own fixed kernel: conv_halo_c32_c64 (3x3/s1, 32 -> 64, with or without a folded shortcut) and darknet-53's 64 -> 128
// downsampling conv, window-staged with its filters in registers (conv_s2.hip).  Reads fused (both stems), residual_from
static void mark_halo_and_s2(yolo_ctx *c)
{
    if (!(ctx16(c) && !getenv("YOLO_NO_HALO"))) return;
    for (int i = 1; i < (int)c->layers.size(); ++i) {
        Layer &L = c->layers[i];
        if (!plain_conv(L) || L.fused != F_NONE || L.size != 3 || L.pad != 1 || !plain16(L) || c->pair_of(L.in[0])) continue;
        if (L.stride == 1 && L.cin == 32 && L.filters == 64 && (L.residual_from < 0 || c->layers[L.residual_from].store_dt == L.in_dt)) L.kernel = K_HALO;
        if (L.stride == 2 && L.cin == 64 && L.filters == 128 && !hosts_shortcut(L) && !getenv("YOLO_NO_S2")) L.kernel = K_S2;
    }
}

// conv3 + shortcut + stride-2 conv in one launch (conv_c3s2.hip): a halo conv whose folded shortcut output (layer i + 1) is read by the s2 conv at i + 2 and by
// nobody else -- that tensor then never leaves LDS.  Both layers keep their own kernels: the fall-back where the fused launch's 32-bit windows do not hold the batch.
// Reads kernel (mark_halo_and_s2), residual_from and noop (fold_shortcuts)
static void mark_c3s2(yolo_ctx *c, const std::vector<int> &uses)
{
    const int NL = (int)c->layers.size();
    if (!(ctx16(c) && !c->keep_layers && !getenv("YOLO_NO_C3S2"))) return;
    for (int i = 1; i + 2 < NL; ++i) {
        Layer &A = c->layers[i], &S = c->layers[i + 1], &B = c->layers[i + 2];
        if (A.kernel == K_HALO && B.kernel == K_S2 && A.residual_from >= 0 && S.type == L_SHORTCUT && S.noop && uses[i] == 1 && uses[i + 1] == 1 && B.in[0] == i + 1 && A.in[0] >= 0 &&
            A.in_dt == B.in_dt && c->layers[A.residual_from].C == 64) { A.fused = B.fused = F_C3S2; A.launcher = B.launcher = i + 2; }
    }
}

// 1x1 convs that can ride in their producer's epilogue: conv i (16-bit, 128 or 256 output channels, optionally with its fused shortcut) read
// by a 1x1/s1 conv with half as many filters.  Reads kernel / fused / launcher of every layer (fixed_kernel, issues_launch), residual_from
static void mark_tails(yolo_ctx *c, const std::vector<int> &uses)
{
    const int NL = (int)c->layers.size();
    if (!(ctx16(c) && !c->keep_layers)) return;
    for (int i = 0; i + 1 < NL; ++i) {
        Layer &P = c->layers[i];
        if (!plain_conv_no_fc(P) || fixed_kernel(P) || (P.filters != 128 && P.filters != 256)) continue;      // (fixed kernels host no tail: run_conv would skip the 1x1)
        if (c->split() && (P.pair || c->pair_of(P.in[0]))) continue;       // (split-fp16 networks: the tail rides on plain fp16 layers only)
        const int o = hosts_shortcut(P) ? i + 1 : i;            // its shortcut was folded into it: consumers read layer i+1
        const int j = o + 1;
        if (j >= NL) continue;
        Layer &T = c->layers[j];
        if (plain_conv_no_fc(T) && T.in[0] == o && conv_is(T, 1, 1, 0) && T.filters * 2 == P.filters &&
            !hosts_shortcut(T) && issues_launch(c, j) && T.in_dt == P.in_dt && !T.pair) { P.tail_layer = j; T.fused_into = i; }      // (same operand type: the tail runs on the producer's MFMA)
        // a detection head (1x1, <= 256 filters, fp32 out, linear) as the tail of the 256-channel 3x3 in front of it when nobody else
        // reads that conv (darknet-53's 52 x 52 head): the head tensor is formed from the tile in LDS, bit-identical to the stand-alone launch
        else if (T.type == L_CONV && plain(T) && !T.fc && T.head && T.in[0] == o && uses[o] == 1 && conv_is(T, 1, 1, 0) && P.filters == 256 && T.filters <= 256 &&
                 P.size == 3 && !hosts_shortcut(P) && T.act == ACT_LINEAR && T.in_dt == P.in_dt && is16(T.in_dt) && j + 1 < NL && c->layers[j + 1].type == L_YOLO) { P.tail_layer = j; T.fused_into = i; }
    }
}

// ---- storage steps ----------------------------------------------------------------------------------------------------------
// elements per pixel of a layer's own tensor (a head's fp32 tensor and a [softmax]'s dense rows have their own widths)
static int storage_width(const Layer &L) { return L.pair ? pair_width(L.C) : roundup(L.C, gran_of(L.store_dt)); }

// [logistic] / [activation]: one k_activate launch over the producer's own tensor where this layer is that tensor's only reader, nobody asked
// to keep every layer, and neither tensor is a window of a concatenation; else a tensor of its own, copied first.
// Reads head (network_kind), fused / launcher (never_stored), uses; writes inplace
static int decide_inplace(yolo_ctx *c, const std::vector<int> &uses)
{
    const int NL = (int)c->layers.size();
    for (int i = 0; i < NL; ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_ACTIVATE) continue;
        const int j = L.in[0];
        bool routed = false;
        for (int r = i + 1; r < NL; ++r) if (c->layers[r].type == L_ROUTE && c->layers[r].in.size() >= 2) for (int q : c->layers[r].in) routed |= q == i;
        if (j >= 0 && c->layers[j].head != L.head) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [logistic] / [activation] of a detection head's fp32 tensor", i);
        if (j < 0 || c->keep_layers || routed || uses[j] != 1) continue;
        const Layer &P = c->layers[j];
        L.inplace = (computes(P) || P.type == L_LOCAL || P.type == L_SHORTCUT || P.type == L_L2NORM || P.type == L_UPSAMPLE || P.type == L_MAXPOOL ||
                     P.type == L_ACTIVATE || P.type == L_LRN || P.type == L_CROP) && !never_stored(P, j);
    }
    return YOLO_OK;
}

// route/concat is never executed where its sources can write straight into a channel window of the concatenation: route[j] = the [route]
// layer j writes into (-1: none), off[j] = at which element offset
struct Placement { std::vector<int> route, off; };

// Reads store_dt, pair, head, cost, noop (fold_shortcuts); writes `at`, copy_inputs / copy_offsets of the routes whose sources must be copied
static int place_route_sources(yolo_ctx *c, Placement &at)
{
    const int NL = (int)c->layers.size();
    at.route.assign(NL, -1); at.off.assign(NL, 0);
    for (int i = 0; i < NL; ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_ROUTE || L.in.size() < 2) continue;
        int off = 0;
        for (int j : L.in) {
            int cj = j < 0 ? c->in_c : c->layers[j].C;
            // (pair tensors: interleaved per 32-channel group, so a source of whole groups at a whole-group offset is a window of the
            //  concatenation like any other tensor; element offset 2 x the channel offset)
            const int gran = L.pair ? 32 : gran_of(L.store_dt);
            bool ok = j >= 0 && at.route[j] < 0 && c->layers[j].type != L_ROUTE && !c->layers[j].head &&
                      !is_head_layer(c->layers[j]) && (cj % gran == 0) && (off % gran == 0) &&
                      c->layers[j].type != L_SOFTMAX && !c->layers[j].cost && !(c->layers[j].type == L_AVGPOOL && c->layers[j].store_dt != L.store_dt);
            // a fused-away conv's real producer is the conv; the shortcut layer itself is what gets placed
            if (ok && c->layers[j].type == L_CONV && j + 1 < NL && c->layers[j + 1].noop && c->layers[j + 1].type == L_SHORTCUT) ok = false;
            if (ok) { at.route[j] = i; at.off[j] = L.pair ? 2 * off : off; }
            else {
                // a copied source (run_layer): granule by granule, or element by element at a channel offset that is no multiple of 8; what the
                // copy kernels do not serve is refused here, not at the first forward
                const int dj = j < 0 ? c->act_dt() : (c->layers[j].head && c->dtype != YOLO_FP32) ? DT_F32 : c->layers[j].store_dt;
                if (dj != L.store_dt) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [route] of layer %d, whose tensor is stored in another type (an fp32 head, map or classifier tensor), is not served", i, j);
                if (L.pair && (cj % 32 || off % 32)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [route] copies the %d channels of layer %d to channel offset %d: on split-fp16 pairs a copied source needs whole 32-channel groups", i, cj, j, off);
                if (L.store_dt == DT_FP8 && (cj % 8 || off % 8)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d: [route] copies the %d channels of layer %d to channel offset %d: in the fp8 configuration a copied source needs multiples of 8", i, cj, j, off);
                L.copy_inputs.push_back(j); L.copy_offsets.push_back(off);
            }
            off += cj;
        }
    }
    return YOLO_OK;
}

static int new_storage(yolo_ctx *c, int stride, int dt, size_t pixels, bool persistent)
{
    Storage s; s.stride = stride; s.dt = dt; s.bytes = pixels * (size_t)stride * dt_size(dt); s.persistent = persistent;
    c->storages.push_back(s); return (int)c->storages.size() - 1;
}

// every layer gets a view: a storage of its own, a window of a concatenation, or an alias of its producer's.  Concatenations first, so
// producers can point into them.  Reads `at`, inplace, head, fused / launcher; writes storages, storage / ch_off, noop
static int create_storages(yolo_ctx *c, const Placement &at)
{
    const int NL = (int)c->layers.size();
    const size_t n = (size_t)c->max_batch;
    for (Layer &L : c->layers)
        if (L.type == L_ROUTE && L.in.size() >= 2) { L.storage = new_storage(c, storage_width(L), L.store_dt, n * L.H * L.W, c->keep_layers); L.ch_off = 0; }
    for (int i = 0; i < NL; ++i) {
        Layer &L = c->layers[i];
        if (is_head_layer(L)) { L.noop = true; L.storage = c->layers[i - 1].storage; L.ch_off = c->layers[i - 1].ch_off; continue; }
        if (L.type == L_ROUTE && L.in.size() == 1) { L.noop = true; int j = L.in[0]; if (j < 0) return fail(c, YOLO_ERR_UNSUPPORTED, "route to network input"); L.storage = c->layers[j].storage; L.ch_off = c->layers[j].ch_off; continue; }
        if (L.type == L_ROUTE) continue;
        if (never_stored(L, i) && !fused_may_fall_back(L)) { L.noop = true; continue; }               // lives in LDS only; a group that may fall back keeps its members' storage
        if (L.type == L_SOFTMAX) { L.storage = new_storage(c, L.C, DT_F32, n, true); continue; }      // dense [n][C] probabilities
        if (L.type == L_ACTIVATE && L.inplace) { L.storage = c->layers[L.in[0]].storage; L.ch_off = c->layers[L.in[0]].ch_off; continue; }
        if (at.route[i] >= 0) { L.storage = c->layers[at.route[i]].storage; L.ch_off = at.off[i]; }
        else if (L.head) L.storage = new_storage(c, roundup(L.C, 4), DT_F32, n * L.H * L.W, true);
        else L.storage = new_storage(c, storage_width(L), L.store_dt, n * L.H * L.W, c->keep_layers);
    }
    return YOLO_OK;
}

// a conv whose shortcut was folded writes the shortcut layer's tensor: its own storage slot is unused (unless it is a window of a
// concatenation).  Reads residual_from, `at`; writes storage / ch_off of the conv, bytes of its former storage
static void redirect_folded_convs(yolo_ctx *c, const Placement &at)
{
    for (int i = 0; i + 1 < (int)c->layers.size(); ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_CONV || !hosts_shortcut(L)) continue;
        if (at.route[i] < 0) c->storages[L.storage].bytes = 0;
        L.storage = c->layers[i + 1].storage; L.ch_off = c->layers[i + 1].ch_off;
    }
}

// liveness: def = first writer, last = last reader of any view of a storage.  Reads storage, noop, fused_into, residual_from, fused / launcher
static void compute_liveness(yolo_ctx *c)
{
    auto read_at = [&](int j, int when) { if (j >= 0 && c->layers[j].storage >= 0) { Storage &s = c->storages[c->layers[j].storage]; s.last = std::max(s.last, when); } };
    for (int i = 0; i < (int)c->layers.size(); ++i) {
        Layer &L = c->layers[i];
        if (L.storage < 0) continue;
        if (!L.noop) { Storage &s = c->storages[L.storage]; s.def = std::min(s.def, L.fused_into >= 0 ? L.fused_into : i); s.last = std::max(s.last, i); }      // (whichever way tail_on is toggled later)
        for (int j : L.in) read_at(j, i);
        if (L.type == L_CONV && L.residual_from >= 0) { Storage &s = c->storages[c->layers[L.residual_from].storage]; s.last = std::max(s.last, i); }
        if (never_stored(L, i))           // its group's launch reads what this layer reads: its input and its shortcut source live until the launcher
            for (int j : {L.in[0], L.residual_from}) read_at(j, L.launcher);
    }
}

// greedy pooled assignment in layer order: a storage takes the largest free buffer when it is first written, gives it back after its last
// reader; persistent ones get a buffer of their own.  Reads def / last / bytes / persistent; writes phys, phys_bytes
static void assign_pool(yolo_ctx *c)
{
    std::vector<int> free_list;
    for (int i = 0; i < (int)c->layers.size(); ++i) {
        for (Storage &s : c->storages) {
            if (s.def != i || s.bytes == 0) continue;
            int pick = -1;
            if (!s.persistent) {
                for (size_t f = 0; f < free_list.size(); ++f)
                    if (pick < 0 || c->phys_bytes[free_list[f]] > c->phys_bytes[free_list[pick]]) pick = (int)f;
            }
            if (pick >= 0) { s.phys = free_list[pick]; free_list.erase(free_list.begin() + pick); c->phys_bytes[s.phys] = std::max(c->phys_bytes[s.phys], s.bytes); }
            else { s.phys = (int)c->phys_bytes.size(); c->phys_bytes.push_back(s.bytes); }
        }
        for (Storage &s : c->storages)
            if (s.last == i && s.phys >= 0 && !s.persistent) free_list.push_back(s.phys);
    }
}

// The planner: the order below is the order the steps depend on each other in (see the headers of the steps for what each reads).
int build_plan(yolo_ctx *c, const std::vector<Section> &secs)
{
    const Section &net = secs[0];
    if (int r = parse_sections(c, secs)) return r;
    heads_to_fp32(c);
    if (int r = classifier_tail(c)) return r;
    if (int r = network_kind(c, net)) return r;
    if (int r = input_norm_and_row_limit(c, net)) return r;
    const std::vector<int> uses = count_uses(c);
    if (int r = fold_shortcuts(c, uses)) return r;
    // Marking passes.  What their order must respect:
    //   * all of them run after fold_shortcuts: they test residual_from (and mark_c3s2 the [shortcut]'s noop), and after network_kind, which sets
    //     `head` along a map chain;
    //   * mark_resblocks, mark_stem and mark_pair_stem do not read each other's marks.  No layer can be claimed twice: a resblock starts at
    //     layer >= 1 with a 1x1 conv of 128 channels, the stems own layers 0 and 1 (3x3) and a 1x1 of 64 -> 32 at layer 2; the stem needs
    //     !in_pair and the pair stem in_pair;
    //   * mark_halo_and_s2 runs after all three: it leaves the members of a fused launch alone (`fused != F_NONE`);
    //   * mark_c3s2 runs after mark_halo_and_s2: it joins layers by their `kernel` (K_HALO at i, K_S2 at i + 2).  It does not ask `fused`: it
    //     can only meet layers mark_halo_and_s2 marked, which were in no fused launch;
    //   * mark_tails runs last: fixed_kernel() of the host asks `kernel` and `fused`, issues_launch() of the 1x1 asks `fused` / `launcher`
    //     (tail_on is false throughout planning, so rides_as_tail() is);
    //   * decide_inplace and create_storages run after every marking pass: never_stored() asks `fused` / `launcher`; compute_liveness reads
    //     fused_into, so it runs after mark_tails.
    mark_resblocks(c, uses);
    mark_stem(c, uses);
    mark_pair_stem(c, uses);
    mark_halo_and_s2(c);
    mark_c3s2(c, uses);
    mark_tails(c, uses);
    // Storage: in-place activations before placement and creation (an in-place layer aliases its producer); placement before creation
    // (producers point into the concatenations); the redirect after creation; liveness over the final views; then the pool.
    if (int r = decide_inplace(c, uses)) return r;
    Placement at;
    if (int r = place_route_sources(c, at)) return r;
    if (int r = create_storages(c, at)) return r;
    redirect_folded_convs(c, at);
    compute_liveness(c);
    assign_pool(c);
    // the recurrent layers' state tensors, in layer order (yolo_get_state): none of them is a member of the pool above
    c->states.clear();
    for (int i = 0; i < (int)c->layers.size(); ++i) if (has_state(c->layers[i])) { c->states.push_back({i, false}); if (c->layers[i].type == L_RECUR && c->layers[i].rkind == RECUR_LSTM) c->states.push_back({i, true}); }
    return YOLO_OK;
}

// ---- recurrent layers: sublayers, launches, parameter blobs ----------------------------------------------------------------------------
// file order of the [connected] sublayers (DN/parser.c:1281-1314): 1 = over the state (`output` inputs), 0 = over the layer's input
int recur_sublayers(const Layer &L, int subs[8])
{
    static const int rnn[3] = {0, 1, 1}, gru[6] = {1, 1, 1, 0, 0, 0}, lstm[8] = {1, 1, 1, 1, 0, 0, 0, 0};      // input self output | wz wr wh uz ur uh | wi wf wo wg ui uf uo ug
    const int n = L.rkind == RECUR_RNN ? 3 : L.rkind == RECUR_GRU ? 6 : 8;
    std::copy(L.rkind == RECUR_RNN ? rnn : L.rkind == RECUR_GRU ? gru : lstm, (L.rkind == RECUR_RNN ? rnn : L.rkind == RECUR_GRU ? gru : lstm) + n, subs);
    return n;
}

// elements per pixel of the tensor layer idx's view lies in (-1: the network input); valid once create_storages ran
static int stride_of(const yolo_ctx *c, int idx) { return idx < 0 ? (c->vec_n ? roundup(c->vec_n, 8) : c->in_pair ? 24 : roundup(c->in_c, 8)) : c->layers[idx].storage >= 0 ? c->storages[c->layers[idx].storage].stride : 0; }

RecurGeom recur_geom(const yolo_ctx *c, const Layer &L)
{
    RecurGeom g; memset(&g, 0, sizeof g);
    g.x_len = L.fc_h * L.fc_w * stride_of(c, L.in[0]); g.s_stride = roundup(L.filters, 8);
    const int kx = roundup(g.x_len, 32), kh = roundup(g.s_stride, 32);
    g.launches = L.rkind == RECUR_LSTM ? 1 : 2;
    g.mode[0] = L.rkind == RECUR_RNN ? RK_RNN_STATE : L.rkind == RECUR_GRU ? RK_GRU_GATES : RK_LSTM; g.Kx[0] = kx; g.Kh[0] = kh;
    if (L.rkind == RECUR_RNN) { g.mode[1] = RK_DENSE; g.Kx[1] = kh; g.Kh[1] = 0; }          // the output sublayer over the new state
    if (L.rkind == RECUR_GRU) { g.mode[1] = RK_GRU_BLEND; g.Kx[1] = kx; g.Kh[1] = kh; }      // [x | r * h]
    for (int q = 0; q < g.launches; ++q) g.Mp[q] = recur_rows(g.mode[q], L.filters);
    return g;
}

size_t state_elems(const yolo_ctx *, const Layer &L) { return L.type == L_CRNN ? (size_t)L.H * L.W * roundup(L.cin, 8) : (size_t)roundup(L.filters, 8); }

size_t recur_blob_bytes(const yolo_ctx *c, const Layer &L, int k)
{
    const RecurGeom g = recur_geom(c, L); const int q = k >> 1;
    if (q >= g.launches) return 0;
    return k & 1 ? (size_t)2 * g.Mp[q] * 4 : (size_t)g.Mp[q] * (g.Kx[q] + g.Kh[q]) * dt_size(L.in_dt);
}

int allocate(yolo_ctx *c)
{
    c->phys.assign(c->phys_bytes.size(), nullptr);
    for (size_t i = 0; i < c->phys_bytes.size(); ++i) {
        HIPCK(c, hipMalloc(&c->phys[i], c->phys_bytes[i] + 256));
        HIPCK(c, hipMemsetAsync(c->phys[i], 0, c->phys_bytes[i] + 256, c->stream));
    }
    for (auto &L : c->layers) {
        L.out.n = c->max_batch; L.out.h = L.H; L.out.w = L.W; L.out.c = L.C;      // geometry even when nothing is stored
        if (L.storage < 0) continue;
        Storage &s = c->storages[L.storage];
        if (s.phys < 0) return fail(c, YOLO_ERR_STATE, "internal: storage without buffer");
        L.out.n = c->max_batch; L.out.h = L.H; L.out.w = L.W; L.out.c = L.C; L.out.stride = s.stride; L.out.dt = s.dt;
        L.out.ptr = (char *)c->phys[s.phys] + (size_t)L.ch_off * dt_size(s.dt);
    }
    // network input: 3 real channels padded to 8; N planes ([net] yolo_input=planes) padded to whole granules
    c->input.dt = c->dtype == YOLO_FP32 ? DT_F32 : (c->dtype == YOLO_FP16 || c->split()) ? DT_F16 : DT_BF16;            // fp8 mode keeps the image in bf16
    const int in_stride = stride_of(c, -1);                    // split fp16: hi | lo | hi blocks of the 8 padded channels; a vector network: [max_batch][roundup(N, 8)], the padding zero
    size_t in_bytes = (size_t)c->max_batch * c->in_h * c->in_w * in_stride * dt_size(c->input.dt) + (c->vec_n ? 256 : 0);      // (+ a tail the 16-byte pieces of a row's reader may touch, as the pool's buffers have)
    HIPCK(c, hipMalloc(&c->input.ptr, in_bytes)); HIPCK(c, hipMemsetAsync(c->input.ptr, 0, in_bytes, c->stream));      // defined even if a timing pass runs before any image was staged
    c->input.n = c->max_batch; c->input.h = c->in_h; c->input.w = c->in_w; c->input.c = c->vec_n ? c->vec_n : c->in_c == 3 ? 8 : c->in_c; c->input.stride = in_stride;
    if (c->split()) {
        // fp32 staging for the layers that run in fp32 between a join and a split (input conversion, upsample, pooling, reorg)
        size_t cap = (size_t)c->max_batch * c->in_h * c->in_w * 8;
        for (auto &L : c->layers) if (L.type == L_UPSAMPLE || L.type == L_MAXPOOL || L.type == L_REORG) {
            const TView in = view_of(c, L.in[0]);
            cap = std::max(cap, (size_t)c->max_batch * in.h * in.w * roundup(in.c, 32));
            cap = std::max(cap, (size_t)c->max_batch * L.H * L.W * roundup(L.C, 32));
        }
        c->f32_cap = cap;
        HIPCK(c, hipMalloc((void **)&c->d_f32a, cap * 4)); HIPCK(c, hipMalloc((void **)&c->d_f32b, cap * 4));
    }
    HIPCK(c, hipMalloc(&c->d_zeros, 4096)); HIPCK(c, hipMemsetAsync(c->d_zeros, 0, 4096, c->stream));
    for (size_t i = 0; i < c->layers.size(); ++i) {
        const Layer &L = c->layers[i];
        if (L.s2d7 && c->in_pair) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %zu: a 7x7 / stride 2 first conv does not read an image stored as split-fp16 pairs", i);
        if (L.s2d7) {
            c->s2d = c->input; c->s2d.h = c->in_h / 2; c->s2d.w = c->in_w / 2; c->s2d.c = 32; c->s2d.stride = 32;
            HIPCK(c, hipMalloc(&c->s2d.ptr, (size_t)c->max_batch * c->s2d.h * c->s2d.w * 32 * dt_size(c->s2d.dt)));
        }
        if (L.fc) {             // the flattened producer must be dense: one pixel of fc_h * fc_w * fc_c contiguous elements per image
            const TView in = view_of(c, L.in[0]);
            // ... or, where the producer is one pixel, that pixel padded to whole granules: anything in a vector network (its input, a recurrent or
            // [connected] layer), and in an image network a [connected] layer (YOLOv1's [connected] behind a [connected] of 37 outputs).  The pad
            // lanes are finite -- the GEMM's epilogue writes act(0) there, a post-activation pass act(0) of that, logistic: 0.5 -- and meet zero
            // filter rows, so they add nothing
            const bool padded_row = c->vec_n || (L.in[0] >= 0 && c->layers[L.in[0]].fc);
            const bool one_pixel = L.fc_h * L.fc_w == 1 && in.c == L.fc_c && in.stride == L.cin_pad && in.dt == L.in_dt && padded_row;
            if (!one_pixel && (in.stride != in.c || in.c != L.fc_c)) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %zu: [connected] needs a dense producer (channels a multiple of 8, not part of a concat)", i);
        }
    }
    c->stage_bytes = (size_t)c->max_batch * c->in_h * c->in_w * (c->vec_n ? c->vec_n : c->in_c) * 4;
    HIPCK(c, hipMalloc(&c->d_stage, c->stage_bytes));
    HIPCK(c, hipMalloc((void **)&c->d_descs, (size_t)c->max_batch * sizeof(ImgDesc)));      // ragged batches: one descriptor per image
    HIPCK(c, hipMalloc((void **)&c->d_frames, (size_t)c->max_batch * sizeof(FrameDesc)));      // ... and one per decoded video frame
    size_t nr = (size_t)c->max_batch * c->rows;
    if (c->rows == 0) nr = 1;            // a classifier or a map network has no candidate rows: the detection workspace is one element each
    if (c->cls_layer >= 0) {
        HIPCK(c, hipMalloc((void **)&c->d_cls_idx, (size_t)c->max_batch * CLS_TOPK_MAX * 4)); HIPCK(c, hipMalloc((void **)&c->d_cls_prob, (size_t)c->max_batch * CLS_TOPK_MAX * 4));
    }
    HIPCK(c, hipMalloc((void **)&c->d_det, nr * (c->attrs ? c->attrs : 1) * 4));
    HIPCK(c, hipMalloc((void **)&c->d_box4, nr * 16));
    HIPCK(c, hipMalloc(&c->d_lean_list, nr * 16)); HIPCK(c, hipMalloc((void **)&c->d_lean_cnt, 4)); HIPCK(c, hipMemsetAsync(c->d_lean_cnt, 0, 4, c->stream));
    for (auto &t : c->trees) if (int r = upload_tree(c, t)) return r;
    c->lean_ok = true;                  // every head a [yolo] head the cell-per-wave decode serves
    for (auto &L : c->layers) {
        if (L.type == L_REGION || L.type == L_DETECT) c->lean_ok = false;
        if (L.type == L_YOLO && L.na * (5 + L.classes) > 256) c->lean_ok = false;
    }
    // ... or the one [region] head with a tree: its descent form writes scores, labels and box4.  Which form yolo_detect* takes:
    // YOLO_TREE_FULL forces the full decode, YOLO_TREE_DESCENT the descent; otherwise TREE_DESCENT_DEFAULT (NOTEBOOK, "Softmax trees")
    c->fragw = !getenv("YOLO_NO_FRAGW");      // (A/B and the identity tests: the same ids with their filter stages in LDS)
    c->tree_full = getenv("YOLO_TREE_FULL") ? true : getenv("YOLO_TREE_DESCENT") ? false : !TREE_DESCENT_DEFAULT;
    if (c->tree_head >= 0) c->lean_ok = !c->tree_full;
    c->lean_heads = 0;
    if (c->lean_ok) {
        int classes = -1; bool same = true;
        for (auto &L : c->layers) if (L.type == L_YOLO) { ++c->lean_heads; same = same && (classes < 0 || classes == L.classes) && L.na <= 16 && 5 + L.classes <= 128; classes = L.classes; }
        if (!same || (size_t)c->max_batch * c->rows * 340 >= 0xffffffffull) c->lean_heads = 0;      // 32-bit element offsets in the kernel
    }
    c->rows_pow2 = 1; while (c->rows_pow2 < c->rows) c->rows_pow2 <<= 1;
    HIPCK(c, hipMalloc((void **)&c->d_scores, nr * 4)); HIPCK(c, hipMalloc((void **)&c->d_labels, nr * 4));
    HIPCK(c, hipMalloc((void **)&c->d_cand, nr * 4)); HIPCK(c, hipMalloc((void **)&c->d_keys, (size_t)c->max_batch * c->rows_pow2 * 8));
    HIPCK(c, hipMalloc((void **)&c->d_sbox, nr * 16)); HIPCK(c, hipMalloc((void **)&c->d_slabel, nr * 4)); HIPCK(c, hipMalloc((void **)&c->d_sscore, nr * 4));
    HIPCK(c, hipMalloc((void **)&c->d_counts, (size_t)c->max_batch * 4));
    // filters
    for (auto &L : c->layers) if (L.type == L_CONV || is_side_conv(L)) {
        size_t wb = filter_bytes(L);
        HIPCK(c, hipMalloc(&L.d_w, wb)); HIPCK(c, hipMemsetAsync(L.d_w, 0, wb, c->stream));
        HIPCK(c, hipMalloc((void **)&L.d_b, (size_t)L.cout_pad * 4)); HIPCK(c, hipMemsetAsync(L.d_b, 0, (size_t)L.cout_pad * 4, c->stream));
        if (L.in_dt == DT_FP8 || L.type == L_XCONV) { HIPCK(c, hipMalloc((void **)&L.d_sc, (size_t)L.cout_pad * 4)); HIPCK(c, hipMemsetAsync(L.d_sc, 0, (size_t)L.cout_pad * 4, c->stream)); }
    }
    size_t keep_bytes = 0;
    for (size_t i = 0; i < c->layers.size(); ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_CRNN) continue;
        const TView in = view_of(c, L.in[0]);
        if (!in.ptr || in.dt != L.in_dt || c->pair_of(L.in[0])) return fail(c, YOLO_ERR_UNSUPPORTED, "layer %zu: [crnn] needs a producer stored in the network's own type (not an fp32 head, map or classifier tensor)", i);
        for (Layer &S : L.sub) {
            const size_t wb = (size_t)S.cout_pad * S.kpad * dt_size(S.in_dt);
            HIPCK(c, hipMalloc(&S.d_w, wb)); HIPCK(c, hipMemsetAsync(S.d_w, 0, wb, c->stream));
            HIPCK(c, hipMalloc((void **)&S.d_b, (size_t)S.cout_pad * 4)); HIPCK(c, hipMemsetAsync(S.d_b, 0, (size_t)S.cout_pad * 4, c->stream));
        }
        const size_t bytes = (size_t)c->max_batch * state_elems(c, L) * dt_size(L.in_dt);          // (+ a tail the conv kernels' 16-byte pieces may touch, as the pool's buffers have)
        for (void **p : {&L.d_h, &L.d_hn, &L.d_rh}) { HIPCK(c, hipMalloc(p, bytes + 256)); HIPCK(c, hipMemsetAsync(*p, 0, bytes + 256, c->stream)); }
        keep_bytes += (size_t)c->max_batch * state_elems(c, L) * 8;
    }
    for (size_t i = 0; i < c->layers.size(); ++i) {
        Layer &L = c->layers[i];
        if (L.type != L_RECUR) continue;
        const TView in = view_of(c, L.in[0]);
        if (!in.ptr || in.dt != L.in_dt || in.stride % 8 || c->pair_of(L.in[0]))
            return fail(c, YOLO_ERR_UNSUPPORTED, "layer %zu: a recurrent layer needs a producer stored in the network's own type (not an fp32 head, map or classifier tensor)", i);
        void **blob[4] = {&L.d_w, (void **)&L.d_b, &L.d_w2, (void **)&L.d_b2};
        for (int k = 0; k < 4; ++k) if (const size_t b = recur_blob_bytes(c, L, k)) { HIPCK(c, hipMalloc(blob[k], b)); HIPCK(c, hipMemsetAsync(*blob[k], 0, b, c->stream)); }
        // state: max_batch streams of s_stride elements each, zero (the columns past the units stay zero for good: the kernels read them as operands)
        const size_t ne = (size_t)c->max_batch * roundup(L.filters, 8), es = dt_size(L.in_dt);
        auto zeroed = [&](void **p, size_t bytes) { hipError_t e = hipMalloc(p, bytes); return e != hipSuccess ? e : hipMemsetAsync(*p, 0, bytes, c->stream); };
        HIPCK(c, zeroed(&L.d_h, ne * es));
        if (L.rkind != RECUR_GRU) HIPCK(c, zeroed(&L.d_hn, ne * es));
        if (L.rkind == RECUR_GRU) { HIPCK(c, zeroed(&L.d_rh, ne * es)); HIPCK(c, zeroed((void **)&L.d_h32, ne * 4)); HIPCK(c, zeroed((void **)&L.d_z, ne * 4)); }
        if (L.rkind == RECUR_LSTM) HIPCK(c, zeroed((void **)&L.d_c, ne * 4));
        keep_bytes += ne * 8;          // (state_keep: d_h and the layer's fp32 tensor, if it has one)
    }
    if (keep_bytes) HIPCK(c, hipMalloc(&c->d_state_keep, keep_bytes));
    for (auto &L : c->layers) if (L.type == L_LOCAL) {
        const size_t wn = (size_t)L.H * L.W * L.filters * L.size * L.size * L.cin;
        HIPCK(c, hipMalloc(&L.d_w, wn * dt_size(L.in_dt))); HIPCK(c, hipMalloc((void **)&L.d_b, (size_t)L.H * L.W * L.filters * 4));
    }
    if (c->dtype != YOLO_FP32)
        for (size_t i = 1; i < c->layers.size(); ++i) {
            const Layer &Y = c->layers[i]; Layer &P = c->layers[i - 1];
            if (Y.type == L_YOLO && P.type == L_CONV && P.head && !P.fc) HIPCK(c, hipMalloc((void **)&P.d_obj, (size_t)c->max_batch * P.H * P.W * Y.na * 4));
        }
    HIPCK(c, hipStreamSynchronize(c->stream));
    // The 16-bit / e4m3 conv kernels address their input with 32-bit buffer offsets: the whole-batch activation window of every conv must
    // stay under 2 GiB (launch_conv_bf16's own check).  Refuse a max_batch that cannot run HERE, with the number that can, instead of a bare
    // 'invalid value' from the first forward (a split-fp16 tensor is 2 x as wide, so 416 x 416 stops above batch 96).
    if (c->dtype != YOLO_FP32)
        for (size_t i = 0; i < c->layers.size(); ++i) {
            const Layer &L = c->layers[i];
            if (L.type != L_CONV || L.fc || L.s2d7 || window_check_skipped(L, (int)i)) continue;     // (fused layers: their launch checks its own windows)
            const TView in = view_of(c, L.in[0]);
            const double per_image = (double)in.h * in.w * in.stride * dt_size(L.in_dt), slack = (std::max(L.pad, 1) + 1.0) * (in.w + 1) * in.stride * dt_size(L.in_dt);
            if (per_image * c->max_batch + slack >= 2147483648.0)
                return fail(c, YOLO_ERR_UNSUPPORTED, "max_batch %d: layer %zu reads %.0f bytes per image%s, and a conv's whole-batch input must stay below 2 GiB (32-bit buffer offsets): at most %d images per context",
                            c->max_batch, i, per_image, c->split() ? " (split fp16 pairs: 2 x the channels)" : "", (int)((2147483648.0 - slack - 1) / per_image));
        }
    return YOLO_OK;
}

}  // namespace yolo_impl

// ---- the planner without a device: yolo_plan_check, yolo_plan_table, yolo_plan_dump -----------------------------------------------
// cfg text -> sections and plan in a context that never sees a device; the message of a refusal is left in c.err
static int plan_text(yolo_ctx &c, std::vector<Section> &secs, const char *cfg_text, int dtype, int max_batch, int keep_layers)
{
    c.dtype = dtype; c.max_batch = max_batch; c.keep_layers = keep_layers;
    std::string perr;
    if (max_batch < 1) { c.err = "max_batch < 1"; return YOLO_ERR_INVALID; }
    if (!parse_cfg(cfg_text, secs, perr)) { c.err = perr; return YOLO_ERR_INVALID; }
    return build_plan(&c, secs);
}
// ... and the text and the message handed back: the text must fit `out`
static int plan_text_out(yolo_ctx &c, int r, const std::string &text, const char *who, const char *what, char *out, size_t out_len, char *err, size_t err_len)
{
    if (r == YOLO_OK && (!out || text.size() + 1 > out_len)) r = fail(&c, YOLO_ERR_INVALID, "%s: the %s needs %zu bytes", who, what, text.size() + 1);
    if (out && out_len) snprintf(out, out_len, "%s", r ? "" : text.c_str());
    if (err && err_len) snprintf(err, err_len, "%s", r ? c.err.c_str() : "");
    return r;
}

extern "C" {

int yolo_plan_check(const char *cfg_text, int dtype, char *err, size_t err_len)
{
    yolo_ctx c; std::vector<Section> secs;
    const int r = plan_text(c, secs, cfg_text, dtype, 1, 0);
    if (err && err_len) snprintf(err, err_len, "%s", r ? c.err.c_str() : "");
    return r;
}

int yolo_plan_table(const char *cfg_text, int dtype, int max_batch, int keep_layers, char *out, size_t out_len, char *err, size_t err_len)
{
    yolo_ctx c; std::vector<Section> secs; std::string text;
    const int r = plan_text(c, secs, cfg_text, dtype, max_batch, keep_layers);
    static const char *const kernels[] = {"tiled", "halo", "s2"}, *const kinds[] = {"none", "stem", "pair-stem", "resblock", "c3s2"};      // ConvKernel, FuseKind
    char line[256];
    for (size_t i = 0; r == YOLO_OK && i < c.layers.size(); ++i) {
        const Layer &L = c.layers[i];
        const Storage *st = L.storage >= 0 ? &c.storages[L.storage] : nullptr;
        snprintf(line, sizeof line, "%zu %s kernel=%s fused=%s launcher=%d residual_from=%d tail_layer=%d storage=%d phys=%d def=%d last=%d\n", i, secs[i + 1].type.c_str(),
                 L.type == L_CONV ? kernels[L.kernel] : "-", kinds[L.fused], L.launcher, L.residual_from, L.tail_layer, L.storage, st ? st->phys : -1, st ? st->def : -1, st ? st->last : -1);
        text += line;
    }
    if (r == YOLO_OK) {
        size_t total = 0; for (size_t b : c.phys_bytes) total += b;
        snprintf(line, sizeof line, "buffers %zu bytes %zu\n", c.phys_bytes.size(), total);
        text += line;
        if (c.in_h != c.in_w) {          // a rectangular network only (the table of a square one is pinned byte for byte): its input, every head's grid, the candidate rows per image
            snprintf(line, sizeof line, "input %dx%d", c.in_h, c.in_w); text += line;
            for (size_t i = 0; i < c.layers.size(); ++i) { const Layer &L = c.layers[i]; if (is_head_layer(L)) { snprintf(line, sizeof line, " head %zu grid %dx%d anchors %d", i, L.H, L.W, L.na); text += line; } }
            snprintf(line, sizeof line, " rows %d\n", c.rows); text += line;
        }
    }
    return plan_text_out(c, r, text, "yolo_plan_table", "table", out, out_len, err, err_len);
}

int yolo_plan_dump(const char *cfg_text, int dtype, int max_batch, int keep_layers, char *out, size_t out_len, char *err, size_t err_len)
{
    yolo_ctx c; std::vector<Section> secs; std::string text;
    int r = plan_text(c, secs, cfg_text, dtype, max_batch, keep_layers);
    char buf[512];
    auto put = [&](const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); text += buf; };
    auto ints = [&](const char *name, const std::vector<int> &v) { put(" %s=[", name); for (size_t k = 0; k < v.size(); ++k) put(k ? ",%d" : "%d", v[k]); text += "]"; };
    for (size_t i = 0; r == YOLO_OK && i < c.layers.size(); ++i) {
        const Layer &L = c.layers[i];
        put("layer %zu %s type=%d H=%d W=%d C=%d", i, secs[i + 1].type.c_str(), (int)L.type, L.H, L.W, L.C); ints("in", L.in);
        put(" filters=%d size=%d stride=%d pad=%d bn=%d act=%d post_act=%d general=%d", L.filters, L.size, L.stride, L.pad, L.bn, L.act, L.post_act, (int)L.general);
        put(" cin=%d cin_pad=%d kpad=%d cout_pad=%d in_dt=%d store_dt=%d pair=%d", L.cin, L.cin_pad, L.kpad, L.cout_pad, L.in_dt, L.store_dt, (int)L.pair);
        put(" residual_from=%d head=%d kernel=%d fused=%d launcher=%d", L.residual_from, (int)L.head, L.kernel, L.fused, L.launcher);
        put(" fc=%d fc_h=%d fc_w=%d fc_c=%d s2d7=%d side=%d sqr=%d", (int)L.fc, L.fc_h, L.fc_w, L.fc_c, (int)L.s2d7, L.side, L.sqr);
        put(" tail_layer=%d fused_into=%d noop=%d", L.tail_layer, L.fused_into, (int)L.noop); ints("copy_inputs", L.copy_inputs); ints("copy_offsets", L.copy_offsets);
        put(" psize=%d pstride=%d ppad=%d up_scale=%a inplace=%d", L.psize, L.pstride, L.ppad, (double)L.up_scale, (int)L.inplace);
        put(" na=%d classes=%d row_off=%d anchors=[", L.na, L.classes, L.row_off); for (size_t k = 0; k < L.anchors.size(); ++k) put(k ? ",%a" : "%a", (double)L.anchors[k]);
        put("] groups=%d temperature=%a pool_fused=%d cost=%d tree=%d storage=%d ch_off=%d\n", L.groups, (double)L.temperature, (int)L.pool_fused, (int)L.cost, L.tree, L.storage, L.ch_off);
        if (L.type == L_RECUR) {          // (a line of its own, on the new layer kind only: the dump of every other cfg is pinned byte for byte)
            const RecurGeom g = recur_geom(&c, L);
            put("recurrent %zu kind=%s units=%d inputs=%d shortcut=%d tanh=%d x_len=%d s_stride=%d launches=%d", i, secs[i + 1].type.c_str(), L.filters, L.cin, L.rshortcut, L.rtanh, g.x_len, g.s_stride, g.launches);
            for (int q = 0; q < g.launches; ++q) put(" launch%d=[mode=%d rows=%d kx=%d kh=%d]", q, g.mode[q], g.Mp[q], g.Kx[q], g.Kh[q]);
            put(" state=own(%s)\n", L.rkind == RECUR_LSTM ? "h,c" : "h");
        }
        if (L.type == L_LRN) put("lrn %zu size=%d lo=%d h=%d alpha=%a beta=%a kappa=%a ghost=%d\n", i, L.size, (L.size - 1) / 2, L.size / 2, (double)L.lrn_alpha, (double)L.lrn_beta, (double)L.lrn_kappa, L.size / 2 < L.C ? L.size / 2 : -1);
        if (L.type == L_CROP) { int h0, w0, c0; Cursor{&c, (int)i, 0, 0, 0}.dims(L.in[0], h0, w0, c0); put("crop %zu from=%dx%d to=%dx%d dh=%d dw=%d adjust=%d\n", i, h0, w0, L.H, L.W, (h0 - L.H) / 2, (w0 - L.W) / 2, (int)L.crop_adjust); }
        if (L.type == L_CRNN) {
            put("recurrent %zu kind=crnn hidden=%d output=%d shortcut=%d launches=3", i, L.cin, L.filters, L.rshortcut);
            for (int q = 0; q < 3; ++q) put(" conv%d=[cin=%d cin_pad=%d kpad=%d filters=%d cout_pad=%d bn=%d act=%d]", q, L.sub[q].cin, L.sub[q].cin_pad, L.sub[q].kpad, L.sub[q].filters, L.sub[q].cout_pad, L.sub[q].bn, L.sub[q].act);
            put(" state=own(%dx%dx%d)\n", L.H, L.W, L.cin);
        }
    }
    for (size_t k = 0; r == YOLO_OK && k < c.storages.size(); ++k) {
        const Storage &s = c.storages[k];
        put("storage %zu def=%d last=%d bytes=%zu phys=%d stride=%d dt=%d persistent=%d\n", k, s.def, s.last, s.bytes, s.phys, s.stride, s.dt, (int)s.persistent);
    }
    if (r == YOLO_OK && c.vec_n)          // (a line of its own, for a vector network only: the dump of every other cfg is pinned byte for byte)
        put("vector_input inputs=%d stride=%d dt=%d streams=%d\n", c.vec_n, roundup(c.vec_n, 8), c.act_dt(), c.max_batch);
    if (r == YOLO_OK) {
        put("context in_h=%d in_w=%d in_c=%d in_pair=%d rows=%d attrs=%d cls_layer=%d map_layer=%d tree_head=%d in_mul=%a in_add=%a weights_count=%zu conv_flops=%a phys_bytes=[",
            c.in_h, c.in_w, c.in_c, (int)c.in_pair, c.rows, c.attrs, c.cls_layer, c.map_layer, c.tree_head, (double)c.in_mul, (double)c.in_add, c.weights_count, c.conv_flops);
        for (size_t k = 0; k < c.phys_bytes.size(); ++k) put(k ? ",%zu" : "%zu", c.phys_bytes[k]);
        text += "]\n";
    }
    return plan_text_out(c, r, text, "yolo_plan_dump", "dump", out, out_len, err, err_len);
}

}  // extern "C"
